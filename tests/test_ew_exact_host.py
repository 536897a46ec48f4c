"""CPU: the contract of tests/test_gpu_ew_exact.py, proved without a GPU for every case of tests/ew_cases.py. Each
case reaches the launch geometry it names under the restated ew_geom / bwd_geometry / reduce_groups / grid_for;
the operands meet the range conditions that make equality the only right answer (16-bit values are small
integers, fp32 sums stay exact in any order, relu and the masks meet exact zeros, the pooled windows tie); the
restated constants equal the source's; and the five elementwise entry points refuse, before any launch, the
channel counts their geometry would serve in part (more than 256 16-byte chunks that are no multiple of 256)."""
import re
from pathlib import Path

import pytest
import torch

import ew_cases as W

ROOT = Path(__file__).resolve().parents[1]
BN_HIP = (ROOT / "argus_amd" / "csrc" / "bn.hip").read_text()
COMMON_H = (ROOT / "argus_amd" / "csrc" / "common.h").read_text()
F32, BF16 = 0, 1
BF16_MAX, F32_MAX = 256, 2 ** 24


def _is_int(t):
    return bool((t == t.round()).all())


EW_IDS = [f"C{c}-px{p}" for c, p, _ in W.EW_CASES]


# ---- regimes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,pixels,reduce_only", W.EW_CASES, ids=EW_IDS)
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_elementwise_case_reaches_its_geometry(dt, C_, pixels, reduce_only):
    E = W.ELEMS[dt]
    want = W.REGIMES[(C_, pixels)][dt]
    b = W.bwd_geometry(C_, E, pixels)
    assert b["rows"] == want["reduce"], (b, want)
    if not reduce_only:
        g = W.ew_geom(C_, E, pixels)
        assert (g["PL"], g["cgroups"], g["rows"], g["ppb"], W.last_block(g, pixels)) == want["apply"], (g, want)
        assert g["cgroups"] * g["CC"] == g["chunks"] and b["cgroups"] * b["CC"] == b["chunks"]  # every channel served
        assert g["rows"] <= W.K_EW_TARGET // g["cgroups"]


def test_the_named_regimes():
    """What the table of tests/ew_cases.py exists for, stated case by case."""
    geo = {(c, p, dt): W.ew_geom(c, W.ELEMS[dt], p) for c, p, ro in W.EW_CASES if not ro for dt in W.ELEMS}
    # one pixel: only pixel lane 0 of one block has work
    for dt in W.ELEMS:
        g = geo[64, 1, dt]
        assert g["rows"] == 1 and [W.lane_pixels(1, g["PL"], pl) for pl in range(g["PL"])] == [1] + [0] * (g["PL"] - 1)
    # 64 x 1541: two kEwU trips a thread, the second partial, in every block and lane
    for dt in W.ELEMS:
        g = geo[64, 1541, dt]
        for npx in (g["ppb"], W.last_block(g, 1541)):
            for pl in range(g["PL"]):
                n, last = W.trips(npx, g["PL"], pl)
                assert n == 2 and 0 < last < W.K_EW_U, (dt, npx, pl, n, last)
    # middle widths: several lanes, several rows
    assert geo[256, 199, "bf16"]["PL"] == 8 and geo[256, 199, "fp32"]["PL"] == 4
    assert geo[256, 199, "bf16"]["rows"] == 2 and geo[256, 199, "fp32"]["rows"] == 4
    # 192 channels: 256 % chunks != 0 leaves 16 spare threads in both types
    for dt in W.ELEMS:
        g = geo[192, 331, dt]
        assert 256 % g["chunks"] != 0 and W.spare_threads(g) == 16 and g["rows"] > 1
    # 2048 channels: one pixel lane; fp32 runs two channel groups
    for px in (64, 67, 8229):
        assert geo[2048, px, "bf16"]["PL"] == 1 and geo[2048, px, "bf16"]["cgroups"] == 1
        assert geo[2048, px, "fp32"]["PL"] == 1 and geo[2048, px, "fp32"]["cgroups"] == 2
    # 67 pixels: the second trip of every block is partial (the clamped loads), the last block shorter still
    for dt in W.ELEMS:
        g = geo[2048, 67, dt]
        assert W.trips(g["ppb"], 1, 0) == (2, 6) and W.trips(W.last_block(g, 67), 1, 0) == (2, 3)
    # 8229 pixels: the 512-block target caps the rows (the 16-pixel minimum alone would give 515)
    assert -(-8229 // (W.K_EW_MIN_PPT * 1)) == 515 > W.K_EW_TARGET
    assert geo[2048, 8229, "bf16"]["rows"] == 485 and W.last_block(geo[2048, 8229, "bf16"], 8229) == 1
    assert geo[2048, 8229, "fp32"]["rows"] == 250 == 500 // 2 and W.last_block(geo[2048, 8229, "fp32"], 8229) == 12
    # the reduce: 25 and 129 rows, and kBwdMaxRows (1026 blocks of 64 pixels wanted)
    assert W.bwd_geometry(64, 8, 1541)["rows"] == 25 and W.bwd_geometry(2048, 8, 8229)["rows"] == 129
    assert -(-65636 // W.K_BWD_MIN_PX) == 1026 > W.K_BWD_MAX_ROWS
    b = W.bwd_geometry(64, 8, 65636)
    assert (b["ppb"], b["rows"]) == (65, 1010)


def test_finalize_cases_reach_their_groups():
    seen = set()
    for c, rows in W.FIN_CASES:
        G, rpg, lens = W.finalize_groups(rows)
        assert sum(lens) == rows and len(lens) == G
        seen.add(G)
    assert seen == {1, 8, 32, 64}
    span = W.K_FIN_LANES * W.K_LOAD_BATCH  # rows of one trip of a block: 4 lanes x 8 loads
    assert span == 32
    assert any(n % span for c, r in W.FIN_CASES for n in W.finalize_groups(r)[2])  # partial trips
    assert any(n > span for c, r in W.FIN_CASES for n in W.finalize_groups(r)[2])  # more than one trip
    G, rpg, lens = W.finalize_groups(513)
    assert (G, rpg) == (32, 17) and lens[-1] == 0 and lens[-2] == 3 and 31 * rpg > 513  # the empty trailing group
    assert (2048, 129) in W.FIN_CASES and 2048 // 64 == 32 and W.reduce_groups(129) == 8
    assert (100, 70) in W.FIN_CASES and 2 * 64 - 100 == 28 and W.reduce_groups(70) == 8
    for c, rows in W.FIN_CASES:  # one ticket counter a 64-channel block
        assert (c + 63) // 64 * 4 <= W.BN_COUNTER_BYTES


def test_pool_cases_reach_their_grids():
    big = [s for s in W.MAXPOOL_CASES if s[:4] == (1, 364, 364, 256)]
    assert big and big[0][4] == ("fp32",)
    ho, wo = W.pool_hw(364, 364)
    assert ho * wo == 33124 and ho * wo * 64 > W.POOL_GRID_CAP * 256 and W.grid_for(ho * wo * 64) == W.POOL_GRID_CAP
    assert W.grid_for(364 * 364 * 64, W.MAXPOOL_BWD_BLOCKS) == W.MAXPOOL_BWD_BLOCKS
    assert 364 * 364 * 256 < 2 ** 31  # the kernels' 32-bit index math
    for n, h, w, c, dts in W.MAXPOOL_CASES:
        for dt in dts:
            ch = c // W.ELEMS[dt]
            assert c % W.ELEMS[dt] == 0 and 256 % ch == 0 and c <= 256  # what the backward serves
    assert any(c // W.ELEMS[dt] == 1 for *_, c, dts in W.MAXPOOL_CASES for dt in dts)
    hws = {hw for _, hw, _ in W.AVG_FWD_CASES}
    assert {1, W.K_LOAD_BATCH - 1, W.K_LOAD_BATCH + 1, 64, 252} <= hws
    assert any(n * c % 256 for n, _, c in W.AVG_FWD_CASES)  # a block that is not full
    n, hw, c, dts = W.AVG_BWD_CASES[-1]
    assert dts == ("bf16",) and n * hw * c // 8 == 2162688 > W.POOL_GRID_CAP * 256


# ---- range conditions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,pixels,reduce_only", W.EW_CASES, ids=EW_IDS)
def test_elementwise_operands_meet_the_contract(C_, pixels, reduce_only):
    c = W.ew_case(C_, pixels)
    for nm, v in c.lo_values().items():
        assert _is_int(v) and v.abs().max().item() <= BF16_MAX, (c, nm, v.abs().max().item())
    for nm, v in c.f32_magnitudes().items():  # in units of 0.5: every partial sum is exact in fp32 in any order
        assert float(v) < 2 ** 23, (c, nm, float(v))
    for nm, v in (("mean", c.mean), ("mean2", c.mean2)):
        assert _is_int(v)
    for v in (c.invstd, c.invstd2):
        assert set(v.tolist()) <= {0.5, 1.0, 2.0}
    for nm, share in c.zero_shares().items():  # relu and the mode-2 mask meet exact zeros
        assert share >= 0.05, (c, nm, share)
    assert (c.msrc == 0).double().mean() >= 0.05 and 0.3 < c.keep.double().mean() < 0.7
    for mode in (1, 2, 3):
        assert 0.1 < (c.dm(mode) != c.dz).double().mean() < 0.7  # the masks mask


@pytest.mark.parametrize("C_,rows", W.FIN_CASES)
def test_finalize_operands_meet_the_contract(C_, rows):
    b = W.BwdFinCase(C_, rows)
    assert _is_int(b.part) and float(b.magnitude()) < F32_MAX  # integer column sums: dgamma / dbeta exact
    for v in (b.gamma, b.invstd, b.mean):  # powers of two: ca exact, cb and cc one fp64 rounding a term
        assert bool((torch.log2(v.abs()) % 1 == 0).all())
    assert b.count > 0 and b.count & (b.count - 1) != 0  # the division by count does round
    for counted in (False, True):
        f = W.FwdFinCase(C_, rows, counted)
        m = f.merge
        assert f.count > 0 and rows * W.FIN_TILE >= f.count
        assert bool((f.part == f.part.float().double()).all())
        # sum x^2 / M2 <= 2^10: the cancellation in Q - S * mean costs at most 10 of fp64's 53 bits
        assert bool((m["M2"] > 0).all()) and float((m["Q"] / m["M2"]).max()) <= 2 ** 10, (C_, rows, counted)
        if counted:
            assert rows == 1 or int((f.n == 0).sum()) == 1
            assert bool((f.part[f.n == 0] == 0).all())
        else:
            assert int(f.n[-1]) < W.FIN_TILE and f.count == (rows - 1) * W.FIN_TILE + int(f.n[-1])  # short last tile


@pytest.mark.parametrize("shape", [s[:4] for s in W.MAXPOOL_CASES], ids=lambda s: "x".join(map(str, s)))
def test_maxpool_windows_tie(shape):
    c = W.maxpool_case(*shape)
    best, idx, ties = c.fwd
    assert _is_int(best) and best.min() >= 0 and best.max() <= BF16_MAX
    n, h, w, ch = shape
    if h * w > 1:  # (the 1 x 1 image's only window holds one valid tap: nothing to tie with)
        assert (ties > 1).double().mean() >= 0.2, (c, (ties > 1).double().mean().item())
    else:
        assert bool((ties == 1).all()) and bool((idx == 4).all())
    # the first valid tap of the top-left window is (1, 1) = 4: a maximum of 0 there names tap 4 or a later one
    corner = idx[:, 0, 0, :]
    assert set(corner.flatten().tolist()) <= {4, 5, 7, 8}
    if h * w * ch >= 64:
        assert int(((best[:, 0, 0, :] == 0) & (corner == 4)).sum()) > 0  # the all-zero corner does occur
    # the hand-written argmax uses every byte value, taps outside the image included
    if c.idx_hand.numel() >= 512:
        assert set(c.idx_hand.flatten().tolist()) == set(range(9))
    assert _is_int(c.dz) and _is_int(c.dz_hand) and c.dz_hand.abs().max() <= 8
    # the scatter conserves what lands inside the image
    inside = torch.zeros_like(c.dout_hand, dtype=torch.bool)
    for k, rs, ts in W._taps(c.ho, c.wo):
        ok = torch.zeros(1, h + 2, w + 2, 1, dtype=torch.bool)
        ok[:, 1:h + 1, 1:w + 1] = True
        inside |= (c.idx_hand == k) & ok[:, rs, ts, :]
    assert float((c.dout_hand * inside).sum()) == float(c.dz_hand.sum())


def test_maxpool_reference_scans_taps_in_order():
    z = torch.zeros(1, 4, 4, 1, dtype=torch.float64)
    best, idx, ties = W.maxpool_ref(z)
    assert idx[0, :, :, 0].tolist() == [[4, 3], [1, 0]] and ties[0, :, :, 0].tolist() == [[4, 6], [6, 9]]
    z[0, 2, 2, 0], z[0, 3, 3, 0] = 5.0, 5.0
    assert W.maxpool_ref(z)[1][0, 1, 1, 0] == 4  # window rows / columns 1..3: (2, 2) is tap 4, (3, 3) tap 8


@pytest.mark.parametrize("n,hw,ch", W.AVG_FWD_CASES + [s[:3] for s in W.AVG_BWD_CASES[-1:]])
def test_avgpool_operands_meet_the_contract(n, hw, ch):
    c = W.AvgCase(n, hw, ch)
    assert _is_int(c.x) and c.x.abs().max() <= 3 and 3 * hw < 2048  # exact in fp16 too, sums exact in fp32
    assert bool((c.feat == c.feat.float().double()).all())


# ---- drift guard ------------------------------------------------------------------------------------------------
def _const(name, text=BN_HIP):
    m = re.search(rf"\b{name}\s*=\s*(\d+)", text)
    assert m, name
    return int(m.group(1))


def test_restated_constants_equal_the_source():
    assert _const("kBwdMinPx") == W.K_BWD_MIN_PX and _const("kBwdMaxRows") == W.K_BWD_MAX_ROWS
    assert _const("kEwTarget") == W.K_EW_TARGET and _const("kEwMinPpt") == W.K_EW_MIN_PPT
    assert _const("kEwU") == W.K_EW_U and _const("kFinLanes") == W.K_FIN_LANES
    m = re.search(r"#ifndef ARGUS_LOAD_BATCH\s*\n#define ARGUS_LOAD_BATCH (\d+)", COMMON_H)
    assert m and int(m.group(1)) == W.K_LOAD_BATCH and "kLoadBatch = ARGUS_LOAD_BATCH" in COMMON_H
    m = re.search(r"return rows < (\d+) \? (\d+) : \(rows < (\d+) \? (\d+) : \(rows < (\d+) \? (\d+) : (\d+)\)\);", BN_HIP)
    assert m, "reduce_groups"
    v = [int(x) for x in m.groups()]
    assert ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]), (None, v[6])) == W.GROUP_THRESHOLDS
    m = re.search(r"grid_for\(int64_t work, int64_t cap = (\d+)\)", BN_HIP)
    assert m and int(m.group(1)) == W.POOL_GRID_CAP
    m = re.search(r"#define ARGUS_MPB_BLOCKS (\d+)", BN_HIP)
    assert m and int(m.group(1)) == W.MAXPOOL_BWD_BLOCKS
    assert _const("kBnCounterBytes", (ROOT / "argus_amd" / "csrc" / "internal.h").read_text()) == W.BN_COUNTER_BYTES


def test_bwd_rows_entry_point_equals_the_restatement():
    from argus_amd._lib import lib

    D = lib().dll
    for c, pixels, _ in W.EW_CASES:
        for dt, E in W.ELEMS.items():
            assert D.argus_bn_bwd_rows(pixels, c) == W.bwd_geometry(c, E, pixels)["rows"], (c, pixels)
    for pixels in (1, 63, 64, 65, 128, 129, 65535, 65536, 65537, 10 ** 6, 2 ** 31 + 5):
        assert D.argus_bn_bwd_rows(pixels, 64) == W.bwd_geometry(64, 8, pixels)["rows"], pixels


# ---- refusals ---------------------------------------------------------------------------------------------------
def _run(D, dt, c):
    """name -> (status, message) of every entry point of the type at channel count c, called with NULL tensors: a
    served width falls through to the pointer check and a refused one must be turned away before it, so nothing is
    launched either way."""
    N, p = None, 64
    if dt == "x8":
        calls = {"bn_apply_x8": lambda: D.argus_bn_apply_x8(p, c, N, N, N, N, N, N, 1, N, N, N, N),
                 "bn_bwd_apply_x8": lambda: D.argus_bn_bwd_apply_x8(p, c, N, N, N, N, N, N, N, N)}
    else:
        code = {"bf16": BF16, "fp32": F32}[dt]
        calls = {"bn_apply": lambda: D.argus_bn_apply(code, p, c, N, N, N, N, N, N, 1, N, N, N),
                 "bn_bwd_reduce": lambda: D.argus_bn_bwd_reduce(code, p, c, N, 0, N, N, N, N, N, N, N, N, N, N, N, N),
                 "bn_bwd_apply": lambda: D.argus_bn_bwd_apply(code, p, c, N, 0, N, N, N, N, N, N, N, N, N, N, N, N, N,
                                                              N, N)}
    return {nm: (fn(), D.argus_last_error()) for nm, fn in calls.items()}


def test_widths_served_in_part_are_refused():
    """More than 256 chunks that are no multiple of 256 (bf16 C = 2560, fp32 C = 1280): ew_geom / bwd_geometry
    would launch chunks / 256 whole channel groups and never touch the channels past them. Every entry point
    answers with a non-zero status and a message naming the channel count, before the pointer checks."""
    from argus_amd._lib import lib

    D = lib().dll
    seen = 0
    for dt, c in W.REFUSED_WIDTHS.items():
        E = 8 if dt == "x8" else W.ELEMS[dt]
        assert c % E == 0 and c // E > 256 and (c // E) % 256 != 0
        for nm, (rc, msg) in _run(D, dt, c).items():
            assert rc != 0 and nm.encode() in msg and str(c).encode() in msg and b"channels" in msg, (nm, dt, c, rc, msg)
            seen += 1
    assert seen == 8  # 3 entry points x 2 types + the 2 x8 forms


def test_served_widths_pass_the_width_check():
    """C = 192 (256 % chunks != 0) and every ResNet width reach the pointer check: 'bad arguments', not the width."""
    from argus_amd._lib import lib

    D = lib().dll
    for c in W.SERVED_WIDTHS + (4096,):
        for dt in ("bf16", "fp32", "x8"):
            for nm, (rc, msg) in _run(D, dt, c).items():
                assert rc != 0 and b"bad arguments" in msg and b"not served" not in msg, (nm, dt, c, rc, msg)
