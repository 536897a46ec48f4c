"""Shared helper of the exact-arithmetic tests of argus_amd/csrc/bn.hip (not a test module; importable without a
GPU): the BatchNorm apply / backward reduce / backward apply kernels, the two ticket finalizes, the max pool and
the average pool.

Geometry. ew_geom, bwd_rows / bwd_geometry, reduce_groups and grid_for are restated here in plain Python from the
constants of bn.hip and common.h, so every case can state which launch geometry it reaches (REGIMES below;
tests/test_ew_exact_host.py proves each statement and guards the constants against drift of the source).

Operands. Integer-valued, built in fp64 from a generator seeded by the case's shape: activations in [-3, 3],
gradients in [-2, 2], apply coefficients scale in {-2, -1, 1, 2}, shift in [-2, 2], residual scale in {-1, 1, 2},
residual shift in [-1, 1]; backward-apply coefficients ca in {+-1, +-2}, cb in {-1, 0, 1}, cc in [-2, 2]; reduce
statistics mean in [-3, 3], invstd in {0.5, 1, 2}. Every product and sum is then exact in fp32 in any order (the
half-integer terms of sum dm * xhat are multiples of 0.5 below 2^23), every stored bf16 value an integer far below
256, and relu and every mask compare against an exact 0 that the recipe does produce. Masks are strict > 0.

References are plain fp64 restatements with no tiling, computed on first use and never modified.
"""
from functools import cached_property, lru_cache

import torch
import torch.nn.functional as F

from exact_cases import assert_same, choice, gen, ints, keep_mask, pack_bits  # noqa: F401 (re-exported)

# ---- the constants of bn.hip / common.h -----------------------------------------------------------------------
K_BWD_MIN_PX, K_BWD_MAX_ROWS, K_EW_TARGET, K_EW_MIN_PPT, K_EW_U, K_FIN_LANES, K_LOAD_BATCH = 64, 1024, 512, 16, 8, 4, 8
GROUP_THRESHOLDS = ((64, 1), (512, 8), (4096, 32), (None, 64))  # rows < 64 -> 1 group, < 512 -> 8, < 4096 -> 32, else 64
POOL_GRID_CAP, MAXPOOL_BWD_BLOCKS = 8192, 2048
BN_COUNTER_BYTES = 16384
ELEMS = {"bf16": 8, "fp32": 4}  # elements of a 16-byte chunk


def _cdiv(a, b):
    return (a + b - 1) // b


def ew_geom(C, E, pixels, target=K_EW_TARGET):
    """bn.hip ew_geom: the grid of bn_apply_kernel and bn_bwd_apply_kernel."""
    chunks = C // E
    CC = min(chunks, 256)
    PL = 256 // CC
    cgroups = chunks // CC
    rows = min(target // cgroups, _cdiv(pixels, K_EW_MIN_PPT * PL))
    rows = max(rows, 1)
    ppb = _cdiv(pixels, rows)
    return dict(CC=CC, PL=PL, cgroups=cgroups, rows=_cdiv(pixels, ppb), ppb=ppb, chunks=chunks)


def bwd_rows(pixels):
    return min(max(_cdiv(pixels, K_BWD_MIN_PX), 1), K_BWD_MAX_ROWS)


def bwd_geometry(C, E, pixels):
    """bn.hip bwd_geometry: the grid of bn_bwd_reduce_kernel (rows is also what argus_bn_bwd_rows returns)."""
    chunks = C // E
    CC = min(chunks, 256)
    ppb = _cdiv(pixels, bwd_rows(pixels))
    return dict(CC=CC, PL=256 // CC, cgroups=chunks // CC, rows=_cdiv(pixels, ppb), ppb=ppb, chunks=chunks)


def reduce_groups(rows):
    for below, groups in GROUP_THRESHOLDS:
        if below is None or rows < below:
            return groups


def grid_for(work, cap=POOL_GRID_CAP):
    return max(1, min(_cdiv(work, 256), cap))


def last_block(g, pixels):
    """Pixels of the last pixel block."""
    return pixels - (g["rows"] - 1) * g["ppb"]


def lane_pixels(npx, PL, pl):
    """How many pixels pixel lane pl walks in a block of npx pixels (one every PL)."""
    return _cdiv(npx - pl, PL) if pl < npx else 0


def trips(npx, PL, pl):
    """(kEwU trips of lane pl, pixels of its last trip)."""
    k = lane_pixels(npx, PL, pl)
    return _cdiv(k, K_EW_U), (k - 1) % K_EW_U + 1 if k else 0


def spare_threads(g):
    """Threads past the last whole pixel lane (256 % CC != 0): they repeat pixels of lane 0 with identical stores."""
    return 256 - g["CC"] * g["PL"]


def finalize_groups(rows):
    """(G, rows per group, rows of each group) of the finalize merge."""
    G = reduce_groups(rows)
    rpg = _cdiv(rows, G)
    return G, rpg, [max(0, min(rows, (g + 1) * rpg) - g * rpg) for g in range(G)]


# ---- the elementwise kernels ----------------------------------------------------------------------------------
# (C, pixels, reduce only)
EW_CASES = [(64, 1, False), (64, 1541, False), (256, 199, False), (192, 331, False), (2048, 64, False),
            (2048, 67, False), (2048, 8229, False), (64, 65636, True)]
# What each case must reach: {(C, pixels): {dtype: {"apply": (PL, cgroups, rows, ppb, last block), "reduce": rows}}}.
# 256 x 199 runs two apply rows in bf16 and four in fp32 (64 chunks: PL = 4, 16 * 4 = 64 pixels a row at least).
REGIMES = {
    (64, 1): {"bf16": {"apply": (32, 1, 1, 1, 1), "reduce": 1}, "fp32": {"apply": (16, 1, 1, 1, 1), "reduce": 1}},
    (64, 1541): {"bf16": {"apply": (32, 1, 4, 386, 383), "reduce": 25},
                 "fp32": {"apply": (16, 1, 7, 221, 215), "reduce": 25}},
    (256, 199): {"bf16": {"apply": (8, 1, 2, 100, 99), "reduce": 4}, "fp32": {"apply": (4, 1, 4, 50, 49), "reduce": 4}},
    (192, 331): {"bf16": {"apply": (10, 1, 3, 111, 109), "reduce": 6},
                 "fp32": {"apply": (5, 1, 5, 67, 63), "reduce": 6}},
    (2048, 64): {"bf16": {"apply": (1, 1, 4, 16, 16), "reduce": 1}, "fp32": {"apply": (1, 2, 4, 16, 16), "reduce": 1}},
    (2048, 67): {"bf16": {"apply": (1, 1, 5, 14, 11), "reduce": 2}, "fp32": {"apply": (1, 2, 5, 14, 11), "reduce": 2}},
    (2048, 8229): {"bf16": {"apply": (1, 1, 485, 17, 1), "reduce": 129},
                   "fp32": {"apply": (1, 2, 250, 33, 12), "reduce": 129}},
    (64, 65636): {"bf16": {"reduce": 1010}, "fp32": {"reduce": 1010}},
}
# refused widths (more than 256 chunks, no multiple of 256) and the widths that stay served
REFUSED_WIDTHS = {"bf16": 2560, "fp32": 1280, "x8": 2560}
SERVED_WIDTHS = (64, 128, 192, 256, 512, 1024, 2048)


def relu(v):
    return v.clamp_min(0)


def row_sums(t, rows, ppb):
    """(pixels, C) -> (rows, C): the sums over the pixel ranges [r * ppb, (r + 1) * ppb) of the reduce's blocks."""
    p, c = t.shape
    pad = torch.zeros(rows * ppb, c, dtype=t.dtype)
    pad[:p] = t
    return pad.view(rows, ppb, c).sum(1)


class EwCase:
    """Operands and fp64 references of bn_apply / bn_bwd_reduce / bn_bwd_apply at (pixels, C)."""

    def __init__(self, C, pixels):
        self.C, self.pixels = C, pixels
        for tag in range(71, 171):  # a small case redraws until relu and the masks meet their share of exact zeros
            self._draw(gen(C, pixels, tag))
            if pixels * C > 4096 or min(self.zero_shares().values()) >= 0.05:
                break

    def _draw(self, g):
        C, pixels = self.C, self.pixels
        s = (pixels, C)
        self.y, self.y2, self.res = ints(s, -3, 3, g), ints(s, -3, 3, g), ints(s, -3, 3, g)
        self.dz = ints(s, -2, 2, g)
        self.keep = keep_mask(s, g)                                   # mode 3: the packed bits
        self.scale, self.shift = choice((-2, -1, 1, 2), C, g), ints((C,), -2, 2, g)
        self.rsc, self.rsh = choice((-1, 1, 2), C, g), ints((C,), -1, 1, g)
        self.ca, self.cb, self.cc = choice((-2, -1, 1, 2), C, g), choice((-1, 0, 1), C, g), ints((C,), -2, 2, g)
        self.ca2, self.cb2, self.cc2 = choice((-2, -1, 1, 2), C, g), choice((-1, 0, 1), C, g), ints((C,), -2, 2, g)
        self.mean, self.invstd = ints((C,), -3, 3, g), choice((0.5, 1, 2), C, g)
        self.mean2, self.invstd2 = ints((C,), -3, 3, g), choice((0.5, 1, 2), C, g)

    def __repr__(self):
        return f"ew C{self.C} px{self.pixels}"

    def zero_shares(self):
        """Share of exact zeros among the pre-ReLU values of each apply form and the mode-2 mask arguments."""
        forms = {"plain": (False, False), "residual": (True, False), "residual, rsc": (True, True)}
        out = {nm: (self.pre(*f) == 0).double().mean().item() for nm, f in forms.items()}
        out["mode 2"] = (self.y * self.scale + self.shift == 0).double().mean().item()
        return out

    # forward apply: relu?(y * a + b [+ res * ra + rb]); plain residual = ra 1, rb 0
    def pre(self, res, rs):
        v = self.y * self.scale + self.shift
        if res:
            v = v + (self.res * self.rsc + self.rsh if rs else self.res)
        return v

    def out(self, res, rs, do_relu):
        v = self.pre(res, rs)
        return relu(v) if do_relu else v

    @cached_property
    def msrc(self):
        """Mode 1's mask source: a stored block output (about half zeros)."""
        return self.out(False, False, True)

    @cached_property
    def arg2(self):
        """Mode 2's mask argument y * S + H."""
        return self.y * self.scale + self.shift

    def dm(self, mode):
        if mode == 0:
            return self.dz
        m = {1: self.msrc > 0, 2: self.arg2 > 0, 3: self.keep}[mode]
        return self.dz * m

    def terms(self, mode, branch=0):
        """(sum dm, sum dm * xhat) terms per pixel, (pixels, C) each."""
        dm = self.dm(mode)
        y, mu, istd = (self.y, self.mean, self.invstd) if branch == 0 else (self.y2, self.mean2, self.invstd2)
        return dm, dm * ((y - mu) * istd)

    def dy(self, mode, branch=0):
        dm = self.dm(mode)
        if branch == 0:
            return self.ca * dm + self.cb * self.y + self.cc
        return self.ca2 * dm + self.cb2 * self.y2 + self.cc2

    # the contract, for tests/test_ew_exact_host.py
    def lo_values(self):
        out = {"y": self.y, "y2": self.y2, "res": self.res, "dz": self.dz}
        for res, rs in ((False, False), (True, False), (True, True)):
            out[f"pre res={res} rs={rs}"] = self.pre(res, rs)
        for br in (0, 1):
            out[f"dy branch {br}"] = self.dy(0, br)  # unmasked: the masked forms replace dm by 0
        return out

    def f32_magnitudes(self):
        """Sums of magnitudes of the reduce's columns in units of 0.5 (the terms are multiples of 0.5)."""
        out = {}
        for br in (0, 1):
            s, t = self.terms(0, br)
            out[f"sum dm {br}"] = 2 * s.abs().sum(0).max()
            out[f"sum dm*xhat {br}"] = 2 * t.abs().sum(0).max()
        return out


@lru_cache(maxsize=2)
def ew_case(C, pixels):
    """The EwCase of a shape: consecutive tests of one shape share it (the large ones are not all kept)."""
    return EwCase(C, pixels)


# ---- the finalize kernels -------------------------------------------------------------------------------------
# (C, rows): G = 1 / 8 / 32 / 64, partial 32-row trips, the empty trailing group at 513 (rpg 17: group 31 starts
# at row 527), 32 column blocks x 8 groups, and a 64-channel block with 28 idle columns
FIN_CASES = [(64, r) for r in (1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4100)] + [(2048, 129), (100, 70)]
FIN_TILE = 7  # elements of a full forward tile


def pow2(n, exps, g, signed=True):
    v = torch.pow(2.0, choice(exps, n, g))
    return v * (choice((-1, 1), n, g) if signed else 1.0)


class BwdFinCase:
    """Synthetic {sum dm, sum dm * xhat} partial rows of argus_bn_bwd_finalize. The rows are integers, gamma, invstd
    and mean signed powers of two: -gi * S and gi2 * T * mean are then exact, each of cb and cc takes one rounding
    a division by count and cc one for its sum, in fp64, however the compiler associates or contracts them."""

    def __init__(self, C, rows):
        self.C, self.rows = C, rows
        g = gen(C, rows, 83)
        self.part = ints((rows, C, 2), -3, 3, g)
        self.count = 37 * rows + 5
        self.gamma, self.mean = pow2(C, (-1, 0, 1), g), pow2(C, (-1, 0, 1, 2), g)
        self.invstd = pow2(C, (-1, 0, 1), g, signed=False)

    @cached_property
    def ref(self):
        S, T = self.part[..., 0].sum(0), self.part[..., 1].sum(0)
        gi = self.gamma * self.invstd
        gi2 = gi * self.invstd
        cb = -gi2 * T / self.count
        cc = -gi * S / self.count + gi2 * T / self.count * self.mean
        return dict(dgamma=T, dbeta=S, ca=gi, cb=cb, cc=cc)

    def magnitude(self):
        return self.part.abs().sum(0).max()


class FwdFinCase:
    """Synthetic {sum, M2} partial rows of argus_bn_finalize. Tile t holds n_t elements (a full tile FIN_TILE; the
    positive layout's last tile is short, the row-count layout draws n_t in [1, FIN_TILE] with one empty row),
    sum_t an integer in [0, 3 n_t] and M2_t an integer in [n_t, 4 n_t] (0 for the empty row)."""

    def __init__(self, C, rows, counted):
        self.C, self.rows, self.counted = C, rows, counted
        g = gen(C, rows, 89, int(counted))
        if counted:
            n = torch.randint(1, FIN_TILE + 1, (rows,), generator=g)
            if rows > 1:
                n[rows // 2] = 0
        else:
            n = torch.full((rows,), FIN_TILE)
            n[-1] = 3
        self.n = n
        self.count = int(n.sum())
        nn = n.double()[:, None]
        u = torch.rand(rows, C, 2, generator=g, dtype=torch.float64)
        self.part = torch.stack([torch.floor(u[..., 0] * (3 * nn + 1)), nn + torch.floor(u[..., 1] * (3 * nn + 1))], -1)
        self.tile_rows = -FIN_TILE if counted else FIN_TILE
        self.gamma = (torch.rand(C, generator=g) + 0.5).double()
        self.beta = ints((C,), -16, 16, g) / 8
        self.rm0, self.rv0 = ints((C,), -32, 32, g) / 8, ints((C,), 1, 32, g) / 8
        self.eps = 1e-5

    @cached_property
    def merge(self):
        """The fp64 merge: S, Q = sum x^2, mean, M2, biased and unbiased variance."""
        s, m2 = self.part[..., 0], self.part[..., 1]
        nn = self.n.double()[:, None]
        S = s.sum(0)
        Q = (m2 + torch.where(nn > 0, s * s / nn.clamp_min(1), torch.zeros_like(s))).sum(0)
        mean = S / self.count
        M2 = Q - S * mean
        var = M2 / self.count
        eps = float(torch.tensor(self.eps, dtype=torch.float32))
        return dict(S=S, Q=Q, mean=mean, M2=M2, var=var, unbiased=M2 / (self.count - 1) if self.count > 1 else var,
                    invstd=1.0 / torch.sqrt(var + eps))


def ulp32(ref):
    """One fp32 unit in the last place at the magnitude of the fp64 value ref (normal range)."""
    return torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23)


# ---- the pools ------------------------------------------------------------------------------------------------
# (n, H, W, C, dtypes): one chunk a pixel in either type; 33,124 output pixels x 64 chunks > 8192 x 256 threads runs
# the grid-stride loop's second trip (and the backward's 2048-block cap)
MAXPOOL_CASES = [(1, 1, 1, 64, ("bf16", "fp32")), (2, 2, 3, 64, ("bf16", "fp32")), (2, 13, 10, 64, ("bf16", "fp32")),
                 (1, 7, 7, 256, ("bf16", "fp32")), (3, 5, 6, 8, ("bf16",)), (3, 5, 6, 4, ("fp32",)),
                 (1, 364, 364, 256, ("fp32",))]
# (n, hw, C): hw below, at +-1 of and well above kLoadBatch; a C that does not fill a block
AVG_FWD_CASES = [(2, 1, 2048), (2, 7, 2048), (2, 9, 6), (3, 64, 2048), (2, 252, 2048)]
AVG_FWD_DTYPES = ("bf16", "fp32", "fp16")
# (n, hw, C, dtypes): 2,162,688 chunks > 8192 x 256 runs the grid-stride loop's second trip
AVG_BWD_CASES = [(2, 64, 2048, ("bf16", "fp32")), (2, 252, 2048, ("bf16", "fp32")), (33, 256, 2048, ("bf16",))]


def pool_hw(h, w):
    return (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1


def _taps(ho, wo):
    """(index, row slice, column slice) of the 9 taps in (r, t) scan order on a tensor padded by one pixel."""
    for r in range(3):
        for t in range(3):
            yield r * 3 + t, slice(r, r + 2 * ho - 1, 2), slice(t, t + 2 * wo - 1, 2)


def maxpool_ref(z):
    """3x3 stride 2 pad 1 max pool of z (n, H, W, C) with -inf padding: (values, index r * 3 + t of the first
    strict maximum in scan order, how many taps reach the maximum)."""
    n, h, w, c = z.shape
    ho, wo = pool_hw(h, w)
    zp = F.pad(z, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    best = torch.full((n, ho, wo, c), float("-inf"), dtype=z.dtype)
    idx = torch.zeros((n, ho, wo, c), dtype=torch.uint8)
    for k, rs, ts in _taps(ho, wo):
        v = zp[:, rs, ts, :]
        take = v > best
        best = torch.where(take, v, best)
        idx = torch.where(take, torch.tensor(k, dtype=torch.uint8), idx)
    ties = torch.zeros((n, ho, wo, c), dtype=torch.uint8)
    for _, rs, ts in _taps(ho, wo):
        ties += (zp[:, rs, ts, :] == best).to(torch.uint8)
    return best, idx, ties


def maxpool_bwd_ref(dout, idx, h, w):
    """Scatter-add of dout (n, Ho, Wo, C) to the tap its index names; a tap outside the image receives nothing."""
    n, ho, wo, c = dout.shape
    dzp = torch.zeros(n, h + 2, w + 2, c, dtype=dout.dtype)
    for k, rs, ts in _taps(ho, wo):
        dzp[:, rs, ts, :] += torch.where(idx == k, dout, torch.zeros_like(dout))
    return dzp[:, 1:h + 1, 1:w + 1, :].contiguous()


class MaxpoolCase:
    """relu(y * scale + shift) pooled 3x3/2: y in [-3, 3], integer coefficients, so about half the pooled values are
    0 and most windows tie."""

    def __init__(self, n, h, w, c):
        self.shape = (n, h, w, c)
        self.ho, self.wo = pool_hw(h, w)
        g = gen(n, h, w, c, 97)
        self.y = ints((n, h, w, c), -3, 3, g)
        self.scale, self.shift = choice((-2, -1, 1, 2), c, g), ints((c,), -2, 2, g)
        self.dout = ints((n, self.ho, self.wo, c), -2, 2, g)
        self.idx_hand = torch.randint(0, 9, (n, self.ho, self.wo, c), generator=g).to(torch.uint8)
        self.dout_hand = ints((n, self.ho, self.wo, c), -2, 2, g)

    def __repr__(self):
        return "maxpool " + "x".join(map(str, self.shape))

    @cached_property
    def fwd(self):
        return maxpool_ref(relu(self.y * self.scale + self.shift))

    @cached_property
    def dz(self):
        return maxpool_bwd_ref(self.dout, self.fwd[1], self.shape[1], self.shape[2])

    @cached_property
    def dz_hand(self):
        return maxpool_bwd_ref(self.dout_hand, self.idx_hand, self.shape[1], self.shape[2])


@lru_cache(maxsize=2)
def maxpool_case(n, h, w, c):
    return MaxpoolCase(n, h, w, c)


class AvgCase:
    def __init__(self, n, hw, c):
        self.shape = (n, hw, c)
        g = gen(n, hw, c, 101)
        self.x = ints((n, hw, c), -3, 3, g)
        self.dfeat = ints((n, c), -2, 2, g)

    @cached_property
    def feat(self):
        """fp32(sum / hw): the fp64 quotient rounded to fp32 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2)."""
        return (self.x.sum(1) / self.shape[1]).float().double()

    def dx(self, tdtype):
        """dfeat * fp32(1 / hw) rounded to the output type: the kernel's two fp32 operations, restated in torch."""
        n, hw, c = self.shape
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hw), dtype=torch.float32)
        return (self.dfeat.float() * inv).to(tdtype).double()[:, None, :].expand(n, hw, c)
