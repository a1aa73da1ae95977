"""Shared by tests/test_gemm_truth_cpu.py and tests/test_gemm_truth_gpu.py: GEMM inputs whose exact
answer is known (DESIGN "GEMM truth tests"), the float64 reference of every epilogue, the
element-by-element comparator and the case table of the GPU file. torch only; imports without a GPU.

A [M,K], W [N,K] and the K-extension operands hold integers in [-2, 2], each entry kept with
probability min(1, sqrt(128 / K)); bias holds integers in [-16, 16]. Every partial sum of
A . W^T (+ A2 . W2^T) + bias in any order is then an integer far below 2^24 (exact in f32, split-K
partials included), and the result fits the 8 significant bits of bf16 (asserted, no exceptions), so
cvals = bf16(acc + bias) loses nothing and the epilogue, which epilogue_row8 evaluates in f32 before
one rounding, has a single right bit pattern that no tile shape, K split or MFMA order can change.
The float64 functions below round (.to(bfloat16), ties to even) at exactly the points
include/ltx_hip.h names. For the GELU rows W, W2 and bias carry a factor 2^-4: y lies on a 1/16 grid
with |16 y| <= 255, at most 511 distinct pre-activations.
"""
import collections
import functools
import math
import types

import torch

SEED = 20
EPI = {"store": 0, "gelu": 1, "gated_residual": 2, "lora": 3, "lora_residual": 4, "gelu_bwd": 5, "accum": 6,
       "lora_dgrad_accum": 7, "store_rowdot": 8}
GATE_VALUES = (0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0)
ALPHA = 0.5
BOOST = 24            # leading K entries set to 2 in three rows of A and of W: nine outputs near 96
MAX_BATCHES = 8
BF16, F64 = torch.bfloat16, torch.float64


# ------------------------------------------------------------------------------------------ rounding
def rbf(x, ties=None):
    """float64 -> bf16 (round to nearest, ties to even) -> float64. ties: a dict whose "up" / "down"
    counts grow by the elements of x that lie exactly half way between two bf16 values and went
    up / down in magnitude-signed order (the cases truncation, round-half-up and a skipped inner
    rounding get wrong)."""
    r = x.to(BF16).double()
    if ties is not None:
        d = x - r
        refl = x + d  # the point opposite r: a bf16 value only if x is the midpoint of two neighbours
        tie = (d != 0) & (refl.to(BF16).double() == refl)
        ties["up"] += int((tie & (r > x)).sum())
        ties["down"] += int((tie & (r < x)).sum())
    return r


def on_bf16_grid(x):
    return bool((x.to(BF16).double() == x).all())


# ------------------------------------------------------------------------------------------- operands
def _ints(rows, cols, gen, K=None):
    x = torch.randint(-2, 3, (rows, cols), generator=gen).float()
    p = min(1.0, math.sqrt(128.0 / (K or cols)))
    if p < 1.0:
        x = x * (torch.rand(rows, cols, generator=gen) < p)
    return x


def _prod(a, w):
    """a . w^T, exact: float64 on the GPU; on the CPU float32, where sums of integers (times one
    power of two) under 2^24 are exact in any order and the product is several times faster"""
    if a.is_cuda:
        return a.double() @ w.double().t()
    return (a.float() @ w.float().t()).double()


@functools.lru_cache(maxsize=None)
def operands(M, N, K, K2, gelu=False, group=False, device="cpu"):
    """A, W (, A2, W2), bias as bf16 on `device`, and .P = A . W^T + A2 . W2^T in float64 (computed
    once per operand set). group: two groups of 256 output columns read A2 at column offsets 0 and
    K2 + 8 (ext_group = (256, K2 + 8)). Asserts conditions 1 and 2 of the construction."""
    gen = torch.Generator().manual_seed(SEED + 7919 * M + 104729 * N + 31 * K + 3 * K2 + gelu + 2 * group)
    sc = 2.0 ** -4 if gelu else 1.0
    A, W = _ints(M, K, gen), _ints(N, K, gen)
    brows = sorted({0, M // 2, M - 1})
    bcols = sorted({0, N // 2, N - 1})
    A[brows, :BOOST] = 2.0
    W[bcols, :BOOST] = 2.0
    bias = torch.randint(-16, 17, (N,), generator=gen).float()
    assert float(bias.min()) != float(bias.max())
    c = types.SimpleNamespace(M=M, N=N, K=K, K2=K2, gelu=gelu, group=group, scale=sc, ext=None, ext_group=None)
    dev = torch.device(device)
    put = lambda t: t.to(BF16).to(dev)  # noqa: E731
    c.A, c.W, c.bias = put(A), put(W * sc), put(bias * sc)
    for t, t16 in ((A, c.A), (W * sc, c.W), (bias * sc, c.bias)):
        assert torch.equal(t, t16.float().cpu())
    P = _prod(c.A, c.W)
    bound = _prod(c.A.abs(), c.W.abs())
    if K2:
        stride = K2 + 8
        A2 = _ints(M, stride + K2 if group else stride, gen, K=K2)  # [M, K2] is a strided view of it
        W2 = _ints(N, K2, gen)
        a2, w2 = put(A2), put(W2 * sc)
        if group:
            assert N == 512
            c.ext, c.ext_group = (a2, w2), (256, stride)
            for g in range(2):
                cols, rows = slice(g * stride, g * stride + K2), slice(g * 256, (g + 1) * 256)
                P[:, rows] += _prod(a2[:, cols], w2[rows])
                bound[:, rows] += _prod(a2[:, cols].abs(), w2[rows].abs())
        else:
            c.ext = (a2[:, :K2], w2)
            P += _prod(a2[:, :K2], w2)
            bound += _prod(a2[:, :K2].abs(), w2.abs())
    c.P = P
    c.bias64 = c.bias.double()
    # 1: every partial sum in every order, in grid units, is an integer below 2^24
    c.bound = (float(bound.max()) + float(c.bias64.abs().max())) / sc
    assert c.bound < 2.0 ** 24, c.bound
    # 2: acc and acc + bias are bf16 values, every one of them (on the GELU grid: |16 y| <= 255)
    c.max_acc = float(P.abs().max()) / sc
    for y in (P, P + c.bias64):
        assert on_bf16_grid(y), "acc + bias leaves the bf16 grid"
        assert float(y.abs().max()) / sc <= 255.0, float(y.abs().max()) / sc
    return c


@functools.lru_cache(maxsize=None)
def aux_operands(M, N, device="cpu"):
    """The [M, N] epilogue inputs, one set per output shape: R (multiples of 0.5 in [-64, 64]), O
    (integers in [-4, 4]), q (int16 over the whole range, from the generator, not from a kernel) and
    gate rows from GATE_VALUES (row stride N + 8; every batch its own row)."""
    gen = torch.Generator().manual_seed(SEED + 3 * M + 5 * N)
    dev = torch.device(device)
    x = types.SimpleNamespace()
    x.R = (torch.randint(-128, 129, (M, N), generator=gen).float() * 0.5).to(BF16).to(dev)
    x.O = torch.randint(-4, 5, (M, N), generator=gen).float().to(BF16).to(dev)
    x.q = torch.randint(-32768, 32768, (M, N), generator=gen).to(torch.int16).to(dev)
    vals = torch.tensor(GATE_VALUES)
    gate = torch.zeros(MAX_BATCHES, N + 8)
    gate[:, :N] = vals[torch.randint(0, len(GATE_VALUES), (MAX_BATCHES, N), generator=gen)]
    for b in range(1, MAX_BATCHES):  # no two consecutive batches share a gate anywhere
        same = gate[b, :N] == gate[b - 1, :N]
        gate[b, :N][same] = -gate[b, :N][same]
    x.gate = gate.to(BF16).to(dev)[:, :N]
    return x


@functools.lru_cache(maxsize=None)
def lora_operands(M, N, r, device="cpu"):
    """f32 U / Wd [M, r], Lb [N, r], A [r, N] of the in-epilogue LoRA epilogues: integers in [-2, 2],
    so the fmaf chain and the product with alpha = 0.5 are exact"""
    gen = torch.Generator().manual_seed(SEED + M + 3 * N + 7 * r)
    dev = torch.device(device)
    mk = lambda *s: torch.randint(-2, 3, s, generator=gen).float().to(dev)  # noqa: E731
    return types.SimpleNamespace(U=mk(M, r), Lb=mk(N, r), Wd=mk(M, r), A=mk(r, N))


def plant_ties(R, t, n=8):
    """R (float64 copy of the residual) with n entries replaced so that R + t lands exactly half way
    between two bf16 values in [128, 256) (spacing 1): x.5 with x odd rounds away from zero, with x
    even towards it; the entries alternate between rounding up and down. They are those with |t|
    nearest 160; R stays a multiple of 0.5 in [-64, 64]."""
    R = R.clone()
    flat = (t.abs() - 160.0).abs().flatten()
    pos = torch.topk(flat, min(8 * n, flat.numel()), largest=False).indices
    i = 0
    for p in pos.tolist():
        tv = float(t.flatten()[p])
        s = 1.0 if tv >= 0 else -1.0
        for j in range(64):
            target = s * (128.5 + ((i % 2) ^ (s < 0)) + 2 * j)
            if abs(target) < 256 and abs(target - tv) <= 64:
                R.view(-1)[p] = target - tv
                i += 1
                break
        if i == n:
            break
    assert i >= 2, "no two elements of t within reach of a bf16 tie"
    return R


# ------------------------------------------------------------------------------------------ reference
GELU_K = math.sqrt(2.0 / math.pi)


def _gelu_u2(y):
    return 2.0 * GELU_K * (y + 0.044715 * y ** 3)


def gelu_tanh64(y):
    """y (1 + tanh u) / 2 as y sigmoid(2u): 1 + tanh u itself cancels to 0 in float64 below
    y = -6.6, where the true value is about -1e-14 and a kernel may rightly return it"""
    return y * torch.sigmoid(_gelu_u2(y))


def gelu_tanh_grad64(y):
    """d/dy of y sigmoid(2u), with 1 - s taken as sigmoid(-2u) (no cancellation in either tail)"""
    s, s1 = torch.sigmoid(_gelu_u2(y)), torch.sigmoid(-_gelu_u2(y))
    return s + y * s * s1 * 2.0 * GELU_K * (1.0 + 3 * 0.044715 * y * y)


def rowdot64(y, O, rpb, hd):
    """delta [B, N / hd, rpb] of LTX_EPI_STORE_ROWDOT: per row and head the sum of y * O"""
    M, N = y.shape
    d = (y * O).view(M // rpb, rpb, N // hd, hd).sum(-1)
    return d.transpose(1, 2).contiguous()


def build(row, device="cpu"):
    """The inputs of one table row and the expected value of every output it writes. Returns a
    namespace: .kw (ops.gemm keyword arguments but for the output buffers), .alias (C starts as R and
    is aux0), .want, a dict of "C" (float64, bf16 values), "aux2" (same), "delta" (float64 of exact
    f32 values), "y" (GELU rows: the pre-activation; C and the code are judged by assert_gelu), and
    .ties, the up / down counts of condition 3 (asserted for every epilogue that adds R)."""
    M, N, rpb, opt = row.M, row.N, row.rpb, row.opt
    c = operands(M, N, row.K, row.K2, row.epi == "gelu", "group" in opt, device)
    x = aux_operands(M, N, device)
    ties = dict(up=0, down=0)
    bias = c.bias if "bias" in opt else None
    y = rbf(c.P + (c.bias64 if bias is not None else 0.0))
    assert M % rpb == 0 and M // rpb <= MAX_BATCHES
    gate = x.gate[:M // rpb]
    gate_rows = lambda: gate.double()[torch.arange(M, device=y.device) // rpb]  # noqa: E731
    kw = dict(a=c.A, w=c.W, bias=bias, epilogue=row.epi, ext=c.ext, ext_group=c.ext_group)
    want, alias, R = {}, False, None
    if row.epi == "store":
        want["C"] = y
    elif row.epi == "gelu":
        want["y"] = y
    elif row.epi == "gated_residual":
        t = rbf(gate_rows() * y, ties)
        R = plant_ties(x.R.double(), t)
        want["C"] = rbf(R + t, ties)
        if "aux2" in opt:
            want["aux2"] = y
        kw.update(aux1=gate, rows_per_batch=rpb)
    elif row.epi == "gelu_bwd":
        # the statement the kernel is already held to bitwise: f32 ((y * q) * f32(2 / 32767)), y * q exact
        want["C"] = ((y.float() * x.q.float()) * (2.0 / 32767.0)).to(BF16).double()
        kw.update(aux0=x.q)
    elif row.epi == "accum":
        R = plant_ties(x.R.double(), y)
        want["C"] = rbf(R + y, ties)
        alias = "alias" in opt
        if "gate" in opt:
            want["aux2"] = rbf(want["C"] * gate_rows(), ties)
            kw.update(aux1=gate, rows_per_batch=rpb)
    elif row.epi == "store_rowdot":
        hd = 32 if "hd32" in opt else 64
        want["C"] = y
        want["delta"] = rowdot64(y, x.O.double(), rpb, hd)
        assert float(want["delta"].abs().max()) < 2.0 ** 24
        kw.update(aux0=x.O, rank=hd, rows_per_batch=rpb)
    elif row.epi in ("lora", "lora_residual", "lora_dgrad_accum"):
        r = [int(o[1:]) for o in opt if o[0] == "r" and o[1:].isdigit()][0]
        lo = lora_operands(M, N, r, device)
        if row.epi == "lora_dgrad_accum":
            t = rbf(y + rbf(ALPHA * (lo.Wd.double() @ lo.A.double()), ties), ties)
            kw.update(aux1=lo.Wd, aux2=lo.A)
            res = "res" in opt
        else:
            t = rbf(y + ALPHA * (lo.U.double() @ lo.Lb.double().t()), ties)
            kw.update(aux1=lo.U, aux2=lo.Lb)
            res = row.epi == "lora_residual"
        if res:
            R = plant_ties(x.R.double(), t)
            want["C"] = rbf(R + t, ties)
        else:
            want["C"] = t
        kw.update(alpha=ALPHA, rank=r)
    else:
        raise ValueError(row.epi)
    if R is not None:
        # 3: the case holds bf16 ties, rounded up and rounded down
        assert ties["up"] >= 1 and ties["down"] >= 1, ties
        assert on_bf16_grid(R) and float(R.abs().max()) <= 64.0 and bool((R * 2 == (R * 2).round()).all())
        kw["aux0"] = R.to(BF16)
    return types.SimpleNamespace(kw=kw, want=want, alias=alias, ties=ties, case=c)


# ----------------------------------------------------------------------------------------- comparator
SENT16 = -21555       # 0xABCD: as bf16 -1.46e-12, no value of any case; as a GELU code gelu' = -1.3
SENT32 = 0x7FC00ABC   # a quiet NaN


class Guarded:
    """An output as a view inside a larger buffer prefilled with a sentinel: two rows above and
    below, eight columns left and right (row stride N + 16), or, dense (the f32 delta), 64 elements
    before and after. untouched() says whether everything around the view still holds the sentinel."""

    def __init__(self, shape, dtype, device, dense=False):
        self.dense, self.shape = dense, tuple(shape)
        wide = dtype == torch.float32
        self.sent = SENT32 if wide else SENT16
        idt = torch.int32 if wide else torch.int16
        if dense:
            n = math.prod(shape)
            self.bits = torch.full((n + 128,), self.sent, dtype=idt, device=device)
            self.view = self.bits[64:64 + n].view(dtype).view(shape)
        else:
            M, N = shape
            self.bits = torch.full((M + 4, N + 16), self.sent, dtype=idt, device=device)
            self.view = self.bits.view(dtype)[2:2 + M, 8:8 + N]

    def untouched(self):
        b = self.bits.clone()
        if self.dense:
            b[64:64 + math.prod(self.shape)] = self.sent
        else:
            b[2:2 + self.shape[0], 8:8 + self.shape[1]] = self.sent
        return bool((b == self.sent).all())


def pattern(bad, tile=(128, 128)):
    """what a 2-D bool mismatch map looks like: the count, the first rows and columns, and whether it
    is whole rows, whole 8-column chunks or inside one tile"""
    idx = bad.nonzero()
    rows, cols = idx[:, 0].unique(), idx[:, 1].unique()
    notes = []
    if bool(bad[rows].all()):
        notes.append("whole rows")
    chunks = bad.view(bad.shape[0], -1, 8) if bad.shape[1] % 8 == 0 else None
    if chunks is not None and bool((chunks.all(-1) == chunks.any(-1)).all()):
        notes.append("whole 8-column chunks")
    th, tw = tile
    if len((rows // th).unique()) == 1 and len((cols // tw).unique()) == 1:
        notes.append("inside tile (%d, %d) of %d x %d" % (int(rows[0]) // th, int(cols[0]) // tw, th, tw))
    return "%d of %d differ; rows %s.. (%d rows), cols %s.. (%d cols)%s" % (
        len(idx), bad.numel(), rows[:8].tolist(), len(rows), cols[:8].tolist(), len(cols),
        "; " + ", ".join(notes) if notes else "")


def assert_truth(out, want, what, guard=None, tile=(128, 128)):
    """torch.equal of an output and the exact reference (float64 `want`, converted to out's dtype
    without loss), and the sentinel around the output untouched. The failure names the count, the
    first rows and columns with both values, and the pattern they form."""
    w = want.to(out.dtype)
    assert out.shape == w.shape, (what, out.shape, w.shape)
    if not torch.equal(out, w):
        bad = ~(out == w)  # a NaN left in the output differs too
        bad2 = bad.reshape(-1, bad.shape[-1])
        idx = bad.nonzero()[:4]
        vals = ["%s got %r want %r" % (tuple(i.tolist()), float(out[tuple(i)]), float(w[tuple(i)])) for i in idx]
        raise AssertionError("%s: %s; first: %s" % (what, pattern(bad2, tile), "; ".join(vals)))
    if guard is not None:
        assert guard.untouched(), "%s: written outside its [%s] view" % (what, ", ".join(map(str, guard.shape)))
    return True


def bf16_steps(a, b):
    """distance of two bf16 tensors in representable values (-0 and +0 are the same value)"""
    def order(t):
        i = t.contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (order(a) - order(b)).abs()


def assert_gelu(out, code, y, what, guard=None, code_guard=None):
    """The GELU rows, through a table over the distinct pre-activations (y on the 1/16 grid, at most
    511 values): every element of `out` within 1 bf16 value of bf16(gelu_tanh(y)) evaluated in
    float64 or of the eager evaluation F.gelu(f32 y, approximate="tanh").to(bf16), the oracle's op
    (-0 in the negative tail, where float64 gives about -1e-14); every int16 code within 1 of
    rint(32767 * clamp(gelu'(y) / 2, -1, 1)) in float64. No element is exempt. Returns the worst
    distance of the output from the float64 value, from the nearer of the two, and of the code."""
    import torch.nn.functional as F
    grid = torch.arange(-255, 256, device=y.device, dtype=F64) / 16.0
    idx = (y * 16.0).round().long() + 255
    assert bool(((idx - 255).double() / 16.0 == y).all()) and int(idx.min()) >= 0 and int(idx.max()) <= 510
    ref64 = gelu_tanh64(grid).to(BF16)
    eager = F.gelu(grid.float(), approximate="tanh").to(BF16)
    d64, dea = bf16_steps(out, ref64[idx]), bf16_steps(out, eager[idx])
    near = torch.minimum(d64, dea)
    worst = [int(d64.max()), int(near.max()), 0]
    if int(near.max()) > 1:
        bad = near > 1
        i = bad.nonzero()[0]
        raise AssertionError("%s: GELU output %s; first y %r got %r want %r (float64) or %r (eager)" % (
            what, pattern(bad), float(y[tuple(i)]), float(out[tuple(i)]), float(ref64[idx][tuple(i)]),
            float(eager[idx][tuple(i)])))
    if code is not None:
        wantq = torch.round(32767.0 * (gelu_tanh_grad64(grid) / 2).clamp(-1, 1)).long()
        dq = (code.long() - wantq[idx]).abs()
        worst[2] = int(dq.max())
        if worst[2] > 1:
            bad = dq > 1
            i = bad.nonzero()[0]
            raise AssertionError("%s: GELU code %s; first y %r got %d want %d" % (
                what, pattern(bad), float(y[tuple(i)]), int(code[tuple(i)]), int(wantq[idx][tuple(i)])))
    for g, n in ((guard, "C"), (code_guard, "code")):
        if g is not None:
            assert g.untouched(), "%s: %s written outside its view" % (what, n)
    return tuple(worst)


# ------------------------------------------------------------------------------------ the case table
Row = collections.namedtuple("Row", "id route M N K K2 epi opt variant rpb label split tile")
# the label templates of the routes, over (epilogue number, rank), as ltx_gemm_describe prints them
SMALL3 = "ltx::gemm_nt_kernel<%d, %d, 3>(ltx::GemmParams)"
SMALL2 = "ltx::gemm_nt_kernel<%d, %d, 2>(ltx::GemmParams)"
T_SPLIT = "ltx::gemm_nt_kernel_t<%d, %d, 256, 8, 1>(ltx::GemmParams)"
T224 = "ltx::gemm_nt_kernel_t<%d, %d, 224, 4, 0>(ltx::GemmParams)"
T256 = "ltx::gemm_nt_kernel_t<%d, %d, 256, 8, 0>(ltx::GemmParams)"
RING = "ltx::gemm_ring_kernel<%%d, %%d, %d, %d>(ltx::GemmParams)"
RING_T2 = (0, 1, 2, 3, 6)
# rows per batch of each M: never a divisor of the tile height where M allows one (8 and 256 have only
# powers of two: 8 runs two batches of 4 inside its one tile, 256 one batch), so gate and delta rows
# meet tiles that straddle a batch boundary
RPB = {8: 4, 200: 50, 256: 256, 300: 100, 1100: 275, 2100: 300, 2200: 440, 3800: 475, 17900: 4475}

# (epilogue, options): the set every route runs at K2 = 0 and K2 = 64
EPILOGUES = (("store", ("bias",)), ("store", ()), ("gelu", ("bias",)), ("gelu", ("bias", "code")),
             ("gated_residual", ("bias",)), ("gated_residual", ("bias", "aux2")), ("gelu_bwd", ()),
             ("accum", ()), ("accum", ("alias",)), ("accum", ("gate",)), ("store_rowdot", ()))


def _table():
    rows = []

    def add(route, label, shape, epi, opt=(), K2=0, variant=0, split=False, tile=(128, 128)):
        M, N, K = shape
        if epi == "store_rowdot":  # N % head dim == 0: the next multiple of 64, still ragged in the 128 / 256 wide tiles
            N = (N + 63) // 64 * 64
            if N % 128 == 0:
                N += 64
        rank = [int(o[1:]) for o in opt if o[0] == "r" and o[1:].isdigit()]
        ident = "%s-%dx%dx%d%s-%s%s%s" % (route, M, N, K, "+%d" % K2 if K2 else "", epi,
                                          "".join("-" + o for o in opt), "-v%d" % variant if variant else "")
        rows.append(Row(ident, route, M, N, K, K2, epi, tuple(opt), variant, RPB[M],
                        label % (EPI[epi], rank[0] if rank else 0), split, tile))

    def full(route, label, shape, **kw):
        for K2 in (0, 64):
            for epi, opt in EPILOGUES:
                add(route, label, shape, epi, opt, K2=K2, **kw)

    full("small3", SMALL3, (300, 136, 128))
    full("small3", SMALL3, (8, 136, 64))
    full("small2", SMALL2, (2100, 2056, 128))
    full("small-splitk", SMALL3, (200, 136, 512), split=True)
    for epi, opt in EPILOGUES:  # K2 = 64 counts as a K tile of the last slice
        add("small-splitk", SMALL3, (256, 512, 2048), epi, opt, K2=64, split=True)
    for epi, opt in (("store", ("bias",)), ("store", ()), ("accum", ()), ("accum", ("alias",)), ("accum", ("gate",))):
        add("t-splitk", T_SPLIT, (1100, 1032, 8192), epi, opt, split=True, tile=(256, 256))
    for M, label, th in ((2200, T224, 224), (3800, T256, 256)):
        full("t%d" % th, label, (M, 4104, 64), tile=(th, 256))
        full("t%d" % th, label, (M, 4104, 128), variant=15, tile=(th, 256))
        for K in (128, 384):
            for K2, t2 in zip((0, 64, 128, 192, 384), RING_T2):
                ring = RING % (th // 32, t2)
                for epi, opt in (EPILOGUES if (K == 128 and K2 in (0, 64)) else
                                 (("store", ("bias",)), ("accum", ()), ("accum", ("gate",)))):
                    add("ring%d" % (th // 32), ring, (M, 4104, K), epi, opt, K2=K2, tile=(th, 256))
    # head dim 32, the in-epilogue LoRA epilogues and the grouped extension: one small, one large route
    for route, label, shape, tile in (("small3", SMALL3, (300, 136, 128), (128, 128)),
                                      ("ring7", RING % (7, 0), (2200, 4104, 128), (224, 256))):
        add(route, label, shape, "store_rowdot", ("hd32",), tile=tile)
        for r in (8, 16, 32):
            add(route, label, shape, "lora", ("bias", "r%d" % r), tile=tile)
            add(route, label, shape, "lora_residual", ("bias", "r%d" % r), tile=tile)
            add(route, label, shape, "lora_dgrad_accum", ("r%d" % r,), tile=tile)
            add(route, label, shape, "lora_dgrad_accum", ("r%d" % r, "res"), tile=tile)
    add("small3", SMALL3, (300, 512, 128), "store", ("bias", "group"), K2=64)
    add("ring7", RING % (7, 1), (17900, 512, 128), "store", ("bias", "group"), K2=64, tile=(224, 256))
    assert len({r.id for r in rows}) == len(rows)
    return rows


ROWS = _table()
# the kernel families the table must name: both stage counts of the 128 x 128 kernel, both split-K
# forms, both heights of gemm_nt_kernel_t, and the ring kernel at both heights and every extension
FAMILIES = ([("small3", False), ("small2", False), ("small-splitk", True), ("t-splitk", True), ("t224", False),
             ("t256", False)] + [("ring%d-%d" % (h, t2), False) for h in (7, 8) for t2 in RING_T2])


def family(row):
    if row.route.startswith("ring"):
        return "%s-%d" % (row.route, row.K2 // 64), row.split
    return row.route, row.split
