"""Shared helper of the exact-arithmetic conv tests (not a test module; importable without a GPU).

Integer-valued operands make every product and every partial sum of a conv exact in the fp32 accumulator in any
summation order, and the result exactly representable in the output type, so a kernel must reproduce the fp64
reference exactly: one dropped, duplicated or mis-indexed term anywhere in the reduction is a failed equality,
at any reduction length. The three range conditions the GPU tests rest on (tests/test_exact_host.py proves
them for every case below, on the CPU):

  * every bf16 output (and every bf16 value a kernel stages) is an integer with |v| <= 256, every fp16 output
    an integer with |v| <= 2048;
  * every fp32 output and every fp32 partial sum stays below 2^24 (checked on the sum of magnitudes, so it
    holds for every summation order and every split);
  * every MX-fp8 operand is an integer with |v| <= 15: four significant bits, exact in e4m3 under any
    power-of-two (E8M0) block scale.

Recipe: activations and gradients are uniform integers in [-2, 2]; weights are +-1 (random sign) where
(j + o) % 16 == 0 over the flattened OHWI reduction index j and the filter o, else 0, so every (tap, channel)
position of the forward and of the data-gradient reduction is non-zero in some filter; BN coefficients, biases
and residuals are small integers. Weight gradients have no 256 cap (fp32 dW): their operands are the dense
integer activations and gradients.
"""
from functools import cached_property

import torch
import torch.nn.functional as F

from infer_shapes import DGRAD_PARITY, FWD_PARITY
from test_gpu_kernels import CONV_SHAPES, DGRAD_BN_CASES, FOLD_CASES, FP8_CASES, GLDS_SHAPES, HALO_SHAPES, X8_CASES

BF16_MAX, F16_MAX, F32_MAX, FP8_MAX = 256, 2048, 2 ** 24, 15


# ---- generators (each draws from an explicit torch.Generator) ------------------------------------------------
def gen(*key):
    """A generator seeded from the case's shape, so the host test and the GPU test build the same operands."""
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, g):
    """Uniform integers in [lo, hi] as fp64."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def choice(values, n, g):
    """n draws from ``values`` (integer BN coefficients) as fp64."""
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def sparse_weights(cout, k, cin, g, period=16):
    """OHWI weights, +-1 where (j + o) % period == 0 over the flattened reduction index j and filter o, else 0."""
    j, o = torch.arange(k * k * cin), torch.arange(cout)
    nz = (j[None, :] + o[:, None]) % period == 0
    sign = torch.randint(0, 2, (cout, k * k * cin), generator=g) * 2 - 1
    return (nz * sign).double().view(cout, k, k, cin)


def dense_weights(cout, k, cin, g):
    """Dense +-1 OHWI weights (short reductions: the stem's 147 terms)."""
    return (torch.randint(0, 2, (cout, k, k, cin), generator=g) * 2 - 1).double()


def keep_mask(shape, g):
    """A random boolean mask (the ReLU mask bits of a block output)."""
    return torch.randint(0, 2, tuple(shape), generator=g).bool()


def pack_bits(keep, per_byte):
    """Mask bits as the kernels read them: ``per_byte`` consecutive channels a byte (8 for bf16, 4 for fp32)."""
    return (keep.reshape(-1, per_byte).int() << torch.arange(per_byte)).sum(1).to(torch.uint8)


# ---- fp64 references (NHWC activations, OHWI weights) --------------------------------------------------------
def pad_of(k):
    return 3 if k == 7 else (1 if k == 3 else 0)


def out_hw(h, w, k, s):
    p = pad_of(k)
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def conv_fwd(x, w, s):
    k = w.shape[1]
    return F.conv2d(_nchw(x), _nchw(w), stride=s, padding=pad_of(k)).permute(0, 2, 3, 1).contiguous()


def conv_dx(x_shape, w, dy, s):
    n, h, ww, c = x_shape
    k = w.shape[1]
    g = torch.nn.grad.conv2d_input((n, c, h, ww), _nchw(w), _nchw(dy), stride=s, padding=pad_of(k))
    return g.permute(0, 2, 3, 1).contiguous()


def conv_dw(x, w_shape, dy, s):
    cout, k, _, cin = w_shape
    g = torch.nn.grad.conv2d_weight(_nchw(x), (cout, cin, k, k), _nchw(dy), stride=s, padding=pad_of(k))
    return g.permute(0, 2, 3, 1).contiguous()


def bn_relu(x, scale, shift):
    """The forward prologue relu(x * scale + shift), strict > 0."""
    return torch.relu(x * scale + shift)


def bn_bwd_apply(dm, y, ca, cb, cc):
    """The BN-backward apply dy = ca * dm + cb * y + cc."""
    return ca * dm + cb * y + cc


def rel(a, b):
    """The tolerance tests' error measure: largest absolute error over the reference's largest magnitude."""
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def assert_same(got, ref, *what):
    """Equality of values, not bit patterns (-0.0 equals 0.0; a NaN, the pre-fill of an unwritten element, equals
    nothing). On failure: how many elements differ and where, since the pattern usually names the defect."""
    g = got.double().reshape(ref.shape)
    if torch.equal(g, ref):
        return
    bad = ~(g == ref)
    idx = bad.nonzero()
    raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements differ; first at {idx[:6].tolist()}: "
                         f"got {g[bad][:6].tolist()}, want {ref[bad][:6].tolist()}; last at {idx[-1].tolist()}")


def mx_fp8_roundtrip(t):
    """t (..., C) with C % 32 == 0, quantised to OCP MX-fp8 along the last dimension as the library does (the
    tightest E8M0 block scale: amax * 2^-e in [224, 448); torch's e4m3 rounding of t / 2^e) and dequantised."""
    b = t.double().reshape(-1, t.shape[-1] // 32, 32)
    amax = b.abs().amax(-1, keepdim=True)
    e = torch.floor(torch.log2(amax.clamp_min(2.0 ** -100)))
    e = e - 8 + (amax / torch.pow(2.0, e) >= 1.75).double()
    scale = torch.pow(2.0, e)
    ok = (amax == 0) | ((amax / scale >= 224) & (amax / scale < 448))
    assert bool(ok.all())
    q = (b / scale).float().to(torch.float8_e4m3fn).double() * scale
    return q.reshape(t.shape)


# ---- one conv with everything its passes, prologues and epilogues read ---------------------------------------
class ConvCase:
    """Operands and fp64 references of one conv (n, h, w, cin, cout, k, stride): forward (plain / BN+ReLU prologue),
    data gradient (plain / accumulated / masked addend / BN-backward epilogue in mask modes 2 and 3, dual branch /
    apply prologue) and weight gradient (plain / input prologue / apply prologue). References are computed on
    first use and never modified."""

    def __init__(self, n, h, w, cin, cout, k, s, tag=0, weights=sparse_weights, act=(-2, 2)):
        self.shape = (n, h, w, cin, cout, k, s)
        self.n, self.h, self.w, self.cin, self.cout, self.k, self.s = self.shape
        self.ho, self.wo = out_hw(h, w, k, s)
        g = gen(*self.shape, tag)
        xs, ys = (n, h, w, cin), (n, self.ho, self.wo, cout)
        self.x = ints(xs, act[0], act[1], g)
        self.wt = weights(cout, k, cin, g)           # OHWI
        self.dy = ints(ys, -2, 2, g)
        # forward prologue: integer scale / shift; zeros occur, so the strict > 0 matters
        self.sc, self.sh = choice((1, 2), cin, g), choice((-1, 0, 1), cin, g)
        # data gradient: an integer buffer to accumulate onto / a masked addend with its mask
        self.add = ints(xs, -2, 2, g)
        self.keep = keep_mask(xs, g)
        # BN-backward epilogue (mean 0, invstd 1: xhat = y): the BN inputs of both branches
        self.yb, self.yb2 = ints(xs, -2, 2, g), ints(xs, -2, 2, g)
        # BN-backward apply prologue on dy
        self.ca = choice((1, 2), cout, g)
        self.cb, self.cc = choice((-1, 0, 1), cout, g), choice((-1, 0, 1), cout, g)
        self.ydy = ints(ys, -2, 2, g)

    def __repr__(self):
        return "conv" + "x".join(map(str, self.shape))

    # staged values
    @cached_property
    def xa(self):
        return bn_relu(self.x, self.sc, self.sh)

    @cached_property
    def dy_ap(self):
        return bn_bwd_apply(self.dy, self.ydy, self.ca, self.cb, self.cc)

    # forward
    @cached_property
    def y(self):
        return conv_fwd(self.x, self.wt, self.s)

    @cached_property
    def y_pro(self):
        return conv_fwd(self.xa, self.wt, self.s)

    # data gradient
    @cached_property
    def dx(self):
        return conv_dx(self.x.shape, self.wt, self.dy, self.s)

    @cached_property
    def dx_ap(self):
        return conv_dx(self.x.shape, self.wt, self.dy_ap, self.s)

    @cached_property
    def mask2(self):
        """Mask mode 2 with scale 1, shift 0: y > 0 (y == 0 masks)."""
        return self.yb > 0

    def dm(self, mode, with_add, apply=False):
        """(dgrad + addend) * mask: mode 2 = recomputed from yb, 3 = the packed bits, 0 = no mask."""
        v = (self.dx_ap if apply else self.dx) + (self.add if with_add else 0)
        return v * {0: 1.0, 2: self.mask2, 3: self.keep}[mode]

    @staticmethod
    def partials(dm, y):
        """The BN-backward column sums {sum dm, sum dm * xhat} with mean 0, invstd 1: (C, 2)."""
        c = dm.shape[-1]
        return torch.stack([dm.reshape(-1, c).sum(0), (dm * y).reshape(-1, c).sum(0)], -1)

    # weight gradient
    @cached_property
    def dw(self):
        return conv_dw(self.x, self.wt.shape, self.dy, self.s)

    @cached_property
    def dw_pro(self):
        return conv_dw(self.xa, self.wt.shape, self.dy, self.s)

    @cached_property
    def dw_ap(self):
        return conv_dw(self.x, self.wt.shape, self.dy_ap, self.s)

    # the contract, for tests/test_exact_host.py
    def lo_values(self, fwd=True, dgrad=True, apply=True):
        """name -> every tensor a kernel stores or stages in the 16-bit type."""
        out = {"x": self.x, "w": self.wt, "dy": self.dy}
        if fwd:
            out.update(y=self.y, xa=self.xa, y_pro=self.y_pro)
        if dgrad:
            out.update(dx=self.dx, dx_add=self.dx + self.add)
            if apply:
                out.update(dy_ap=self.dy_ap, dx_ap=self.dx_ap, dx_ap_add=self.dx_ap + self.add)
        return out

    def f32_magnitudes(self, dgrad=True, wgrad=True):
        """name -> sum of the magnitudes of the terms of every fp32 sum (an upper bound of every partial sum)."""
        out = {"fwd acc": self.wt.abs().reshape(self.cout, -1).sum(1).max() * max(self.x.abs().max(), self.xa.max())}
        if dgrad:
            dyx = max(self.dy.abs().max(), self.dy_ap.abs().max())
            out["dgrad acc"] = self.wt.abs().sum((0, 1, 2)).max() * dyx
            for nm, v in (("plain", self.dx + self.add), ("apply", self.dx_ap + self.add)):
                out[f"part sum dm {nm}"] = v.abs().reshape(-1, self.cin).sum(0).max()
                for y in (self.yb, self.yb2):
                    out[f"part sum dm*y {nm}"] = (v * y).abs().reshape(-1, self.cin).sum(0).max()
        if wgrad:
            px = self.n * self.ho * self.wo * self.k * self.k
            out["dw"] = torch.tensor(float(px)) * max(self.x.abs().max(), self.xa.max()) * self.dy_ap.abs().max()
        return out


class StemCase(ConvCase):
    """The 7x7 stride-2 stem (3 -> 64): activations in {-1, 0, 1}, dense +-1 weights, 147 terms."""

    def __init__(self, n, h, w):
        super().__init__(n, h, w, 3, 64, 7, 2, tag=7, weights=dense_weights, act=(-1, 1))


class P1x1Case:
    """A bottleneck conv1's data gradient as the persistent kernel runs it (k1 -> cout = 4 * w3 channels): apply
    prologue on dm1, addend dh, mask bits, BN-backward epilogue on y3 (stored, or recomputed as conv3(a2) from
    a2 (P, w3) and conv3's forward weights) and the downsample branch's yd."""

    def __init__(self, n, hw, w3, k1):
        self.n, self.hw, self.w3, self.k1, self.cout = n, hw, w3, k1, 4 * w3
        self.P = P = n * hw * hw
        g = gen(n, hw, w3, k1, 43)
        self.w1 = sparse_weights(k1, 1, self.cout, g)      # conv1: 4*w3 -> k1 (OHWI)
        self.w3f = sparse_weights(self.cout, 1, w3, g)     # conv3: w3 -> 4*w3
        self.a2 = ints((n, hw, hw, w3), 0, 2, g)           # a ReLU output
        self.dm1, self.y1 = ints((n, hw, hw, k1), -2, 2, g), ints((n, hw, hw, k1), -2, 2, g)
        self.ca = choice((1, 2), k1, g)
        self.cb, self.cc = choice((-1, 0, 1), k1, g), choice((-1, 0, 1), k1, g)
        self.dh = ints((n, hw, hw, self.cout), -2, 2, g)
        self.yd = ints((n, hw, hw, self.cout), -2, 2, g)
        self.keep = keep_mask((n, hw, hw, self.cout), g)

    def __repr__(self):
        return f"p1x1 n{self.n} hw{self.hw} {self.k1}->{self.cout} (y from {self.w3})"

    @cached_property
    def y3(self):
        return conv_fwd(self.a2, self.w3f, 1)

    @cached_property
    def dy1(self):
        return bn_bwd_apply(self.dm1, self.y1, self.ca, self.cb, self.cc)

    @cached_property
    def dx(self):
        return conv_dx((self.n, self.hw, self.hw, self.cout), self.w1, self.dy1, 1)

    def dm(self, with_add):
        return (self.dx + (self.dh if with_add else 0)) * self.keep

    def lo_values(self):
        return {"a2": self.a2, "w1": self.w1, "w3": self.w3f, "dm1": self.dm1, "dy1": self.dy1, "y3": self.y3,
                "dx": self.dx, "dx_add": self.dx + self.dh}

    def f32_magnitudes(self):
        v = self.dx + self.dh
        return {"part sum dm": v.abs().reshape(-1, self.cout).sum(0).max(),
                "part sum dm*y3": (v * self.y3).abs().reshape(-1, self.cout).sum(0).max(),
                "part sum dm*yd": (v * self.yd).abs().reshape(-1, self.cout).sum(0).max()}


class InferCase:
    """A frozen conv: y = relu?(conv(x, w_fold) + bias [+ residual]) and its data gradient
    dx = (conv_dx(dy) [+ addend]) [* (mask > 0)], with w_fold given directly as the integer weights."""

    def __init__(self, n, h, w, cin, cout, k, s):
        self.shape = (n, h, w, cin, cout, k, s)
        self.n, self.h, self.w, self.cin, self.cout, self.k, self.s = self.shape
        self.ho, self.wo = out_hw(h, w, k, s)
        g = gen(*self.shape, 99)
        self.x = ints((n, h, w, cin), -2, 2, g)
        self.wt = sparse_weights(cout, k, cin, g)
        self.bias = ints((cout,), -3, 3, g)
        self.res = ints((n, self.ho, self.wo, cout), -4, 4, g)
        self.dy = ints((n, self.ho, self.wo, cout), -2, 2, g)
        self.add = ints((n, h, w, cin), -2, 2, g)
        self.mask = ints((n, h, w, cin), -1, 1, g)  # a third zeros: > 0, not >= 0

    def __repr__(self):
        return "infer" + "x".join(map(str, self.shape))

    @cached_property
    def y(self):
        return conv_fwd(self.x, self.wt, self.s) + self.bias

    def out(self, use_res, relu):
        v = self.y + self.res if use_res else self.y
        return v.clamp_min(0) if relu else v

    @cached_property
    def dx(self):
        return conv_dx(self.x.shape, self.wt, self.dy, self.s)

    def dx_out(self, use_add, use_mask):
        v = self.dx + self.add if use_add else self.dx
        return v * (self.mask > 0) if use_mask else v

    @cached_property
    def wt_dgrad(self):
        """What argus_conv_fold_bn_dgrad stores: [c][R-1-r][S-1-s][k]."""
        return self.wt.permute(3, 1, 2, 0).flip(1, 2).contiguous()


# ---- case tables -------------------------------------------------------------------------------------------
def _sq(cin, cout, k, s, hin, n):
    return (n, hin, hin, cin, cout, k, s)


IGEMM_CASES = [_sq(cin, cout, k, s, hin, 2) for cin, cout, k, s, hin in CONV_SHAPES]          # all 22, n = 2
GLDS_CASES = [_sq(*sh) for sh in GLDS_SHAPES]
GLDS_RING_CASES = [(8, 12, 12, 256, 1024, 1, 1), (8, 14, 14, 128, 128, 3, 1)]                  # two- vs three-stage ring
# the halo kernel tiles 256 consecutive pixels as whole rows or whole images (12 x 21 does not tile: not served);
# the non-square frame 16 x 32 gives 8-row tiles, two an image
HALO_CASES = [(n, hw, hw, cin, cout, 3, 1) for cin, cout, hw, n in HALO_SHAPES] + [(2, 16, 32, 64, 128, 3, 1)]
# (shape, tuning, kernel name): every kernel family a data gradient with a BN-backward epilogue can land on
DGRAD_BN_EXACT = [(_sq(cin, cout, k, s, hin, n), tune, kname) for cin, cout, k, s, hin, n, tune, kname in DGRAD_BN_CASES]
DGRAD_BN_EXACT += [(_sq(cin, cout, k, s, hin, n), tune, None) for cin, cout, k, s, hin, n, tune in FOLD_CASES]
# 1x1 shapes whose data gradient stages the apply prologue itself (argus_conv_dgrad_stages_prologue == 1)
DGRAD_BN_EXACT += [((2, 16, 16, 256, 64, 1, 1), {}, "igemm_kernel"), ((2, 6, 6, 1024, 256, 1, 1), {}, "igemm_kernel")]
# (n, hw, w3, k1, dual): the persistent conv1 data gradient with the stored y (k1 -> 4 * w3 channels)
P1X1_STORED = [(5, 12, 64, 64, False), (5, 9, 64, 64, True), (5, 8, 128, 128, True), (5, 5, 256, 256, False),
               (5, 7, 256, 256, True)]
# the y recompute: 75 pixels (two tiles, the last ragged), 432, 18,000 (some workgroups walk two tiles); k = 128
# stays on the register-staged igemm, which recomputes y in its epilogue
P1X1_YREC = [(3, 5, 64, 64), (3, 12, 64, 64), (5, 60, 64, 64), (3, 6, 128, 128)]
DGW_CASES = [(2, 33, 33), (1, 5, 7), (8, 64, 64)]                                               # 64 -> 256, 1x1
WGRAD_HALO_CASES = [(1, 64, 64, 64, 64), (1, 32, 32, 128, 128), (2, 16, 16, 64, 128), (4, 8, 8, 128, 64),
                    (1, 16, 16, 256, 128), (1, 10, 84, 64, 64), (1, 7, 168, 128, 128), (2, 12, 21, 64, 64),
                    (1, 47, 84, 128, 128)]                                                      # (n, h, w, cin, cout)
WGRAD_DMA_CASES = [(1, 8, 8, 128, 128), (2, 7, 9, 256, 128), (2, 14, 14, 128, 512), (1, 5, 3, 512, 256),
                   (2, 56, 56, 256, 256), (3, 13, 11, 1024, 256)]                               # (n, h, w, cin, cout)
WGRAD_GATHER_CASES = [(2, 16, 16, 128, 128, 3, 2), (2, 15, 9, 256, 512, 1, 2), (3, 13, 7, 128, 256, 3, 2),
                      (1, 8, 8, 512, 128, 3, 2), (1, 12, 21, 1024, 256, 1, 2)]
FP8_EXACT = [_sq(*sh) for sh in FP8_CASES]
X8_EXACT = [(n, h, w, c, k, 3, 1) for n, h, w, c, k in X8_CASES]
INFER_FWD = list(FWD_PARITY)
INFER_DGRAD = list(DGRAD_PARITY)
STEM_CASES = [(3, 38, 30), (2, 100, 248)]

_CACHE = {}


def conv_case(shape):
    """The ConvCase of a shape, built once and shared (read-only) by every test that needs it."""
    if shape not in _CACHE:
        _CACHE[shape] = ConvCase(*shape)
    return _CACHE[shape]


def wgrad_case(n, h, w, cin, cout, k=1, s=1):
    return conv_case((n, h, w, cin, cout, k, s))
