"""Shared helper of the frozen-conv tests (not a test module; importable without a GPU): the kernel-parity shape
tables of tests/test_gpu_infer.py (the fp16 file imports the same) and tests/test_gpu_frozen_grad.py, the Python
mirror of the library's tile-height rule, and the classification of a conv into the kernel class it launches.

The mirror is held to the library by the GPU tests: every parity case asserts that the kernel it launched is the
instantiation conv_kernel_name() names. tests/test_infer_host.py uses the classification to require that every
class a deployed session launches also occurs among the tables below.
"""
import ctypes as C

# (n, h, w, cin, cout, k, stride): the smallest shapes that reach each failure mode
FWD_PARITY = [
    (1, 6, 10, 64, 64, 1, 1),    # M = 60: below one tile
    (3, 5, 7, 192, 64, 3, 1),    # ragged M, borders on every side, channels not a power of two
    (2, 7, 9, 128, 192, 3, 2),   # odd frame, output 4 x 5
    (2, 9, 7, 256, 128, 1, 2),   # the downsample kind
    (2, 8, 8, 512, 512, 3, 1),   # the layer-4 shape that motivates the split
    # 64-row tiles (cdiv(M, 64) * (cout / 64) >= 256), the last row tile ragged
    (1, 19, 25, 64, 2048, 1, 1),   # M = 475 = 7*64 + 27: the last tile's upper 32-row half is empty
    (1, 37, 49, 128, 2048, 1, 2),  # the downsample kind, output 19 x 25
    (2, 13, 19, 64, 2048, 3, 1),   # M = 494 = 7*64 + 46: 3x3 borders, an image boundary inside a 64-row tile
    (1, 41, 45, 64, 2048, 3, 2),   # 3x3 stride 2, odd frame, output 21 x 23 = 483 = 7*64 + 35
    (2, 32, 32, 128, 512, 1, 1),   # layer2.*.conv3 at 256 x 256, B = 1: exactly on the threshold (32 * 8 = 256)
    (2, 32, 31, 128, 512, 1, 1),   # its neighbour below (31 * 8 = 248): 32-row tiles, a 496-tile unsplit grid
    # classes of the deployed sessions that tests/test_infer_host.py's coverage found in no shape above
    (2, 9, 7, 256, 64, 1, 1),      # 1x1 s1 on 32-row tiles, split by default (layers 3-4): M = 126
    (2, 13, 19, 64, 576, 3, 1),    # 3x3 s1 on 32-row tiles, too many to split (16 x 9 = 144 > 128): layers 1-2
    (3, 19, 25, 64, 640, 3, 2),    # 3x3 s2 likewise (13 x 10 = 130 tiles): layer2.0.conv2; output 10 x 13, M = 390
    (1, 37, 49, 128, 576, 1, 2),   # 1x1 s2 likewise (15 x 9 = 135 tiles): layers 3.0 / 4.0 downsample; output 19 x 25
]

# the data gradient's GEMM is the mirror: M = n*h*w rows, N = cin columns, reduction over k*k*cout
DGRAD_PARITY = [
    (1, 6, 10, 64, 64, 1, 1),    # M = 60: below one tile
    (3, 5, 7, 192, 64, 3, 1),    # ragged M, borders on every side, channels not a power of two
    (2, 7, 9, 128, 192, 3, 2),   # odd frame, output 4 x 5: the stride predicate with padding
    (2, 9, 7, 256, 128, 1, 2),   # the downsample kind: three quarters of dx has no tap
    (2, 8, 8, 512, 512, 3, 1),   # the layer-4 shape that motivates the split
    # 64-row tiles (cdiv(n*h*w, 64) * (cin / 64) >= 256)
    (1, 19, 25, 2048, 64, 1, 1),   # ragged last tile
    (1, 19, 25, 2048, 128, 1, 2),  # 1x1 s2: three quarters of dx has no tap, across two staged rows per thread
    (2, 13, 19, 2048, 64, 3, 1),   # borders and an image boundary inside a tile
    (1, 19, 25, 2048, 64, 3, 2),   # the stride predicate with padding at 64 rows, output 10 x 13
    (2, 64, 64, 128, 128, 3, 2),   # layer2.0.conv2 at 256 x 256, B = 1: exactly on the threshold (128 * 2 = 256)
    # classes of the deployed sessions that tests/test_infer_host.py's coverage found in no shape above
    (2, 9, 7, 64, 256, 1, 1),      # 1x1 s1 on 32-row tiles, split by default (layers 3-4): M = 126
    (2, 13, 19, 576, 64, 3, 1),    # 3x3 s1 on 32-row tiles, too many to split (16 x 9 = 144 > 128): layers 1-2
    (1, 19, 25, 576, 64, 3, 2),    # 3x3 s2 likewise (15 x 9 = 135 tiles): layers 3.0 / 4.0 conv2
    (1, 19, 25, 576, 128, 1, 2),   # 1x1 s2 likewise: layer4.0.downsample in fp32
]

CTYPE = {"fp32": "float", "bf16": "__bf16", "fp16": "_Float16"}


def cdiv(a, b):
    return -(-a // b)


def out_hw(h, w, k, s):
    p = 1 if k == 3 else 0
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def gemm_mn(direction, n, h, w, cin, cout, k, s):
    """(M, N) of the GEMM a conv runs: forward rows are output pixels and columns cout; the data gradient's rows
    are dx pixels and its columns cin."""
    if direction == "fwd":
        ho, wo = out_hw(h, w, k, s)
        return n * ho * wo, cout
    return n * h * w, cin


def infer_bm(M, N):
    """The library's infer_bm(): 64-row tiles once they give each of the 256 CUs a tile, 32-row tiles below."""
    return 64 if cdiv(M, 64) * (N // 64) >= 256 else 32


def conv_kernel_name(direction, dt, shape):
    """The instantiation name (as the kernel timer reports it) a conv of ``shape`` launches."""
    fam = "conv_infer_kernel" if direction == "fwd" else "conv_infer_dgrad_kernel"
    return f"argus::{fam}<{CTYPE[dt]}, {infer_bm(*gemm_mn(direction, *shape))}>"


def is_frozen_conv(name):
    return name.startswith("argus::conv_infer_kernel<") or name.startswith("argus::conv_infer_dgrad_kernel<")


def default_splits(L, direction, dtype_code, shape):
    """The split the library chooses by default, from argus_conv_infer_splits / argus_conv_infer_dgrad_plan
    (host-side planning: no GPU). ``L``: argus_amd._lib.lib()."""
    from argus_amd._lib import ConvDesc

    n, h, w, cin, cout, k, s = shape
    ho, wo = out_hw(h, w, k, s)
    d = ConvDesc(n, h, w, cin, cout, k, k, s, 1 if k == 3 else 0, ho, wo, 0)
    if direction == "fwd":
        sp = L.dll.argus_conv_infer_splits(C.byref(d), dtype_code)
    else:
        v, mx, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
        L.conv_infer_dgrad_plan(C.byref(d), dtype_code, 0, C.byref(v), C.byref(mx), C.byref(nb))
        sp = v.value
    assert sp >= 1, (direction, shape)
    return sp


def conv_class(L, direction, dt, dtype_code, shape):
    """(direction, "fp32" | "16-bit", kernel size, stride, tile rows, default splits > 1)."""
    bm = infer_bm(*gemm_mn(direction, *shape))
    return (direction, "fp32" if dt == "fp32" else "16-bit", shape[5], shape[6], bm,
            default_splits(L, direction, dtype_code, shape) > 1)


def session_convs(batch, hw, n_cams=2):
    """name -> (n, h, w, cin, cout, k, stride) of every folded conv of a session plan: resnet50_blocks() with the
    arithmetic of InferenceSession._plan."""
    from argus_amd.engine import _out, resnet50_blocks

    n = batch * n_cams
    h, w = (_out(_out(x, 7, 2, 3), 3, 2, 1) for x in hw)
    convs = {}
    for b in resnet50_blocks():
        pf = b.prefix
        convs[pf + ".conv1"] = (n, h, w, b.cin, b.width, 1, 1)
        convs[pf + ".conv2"] = (n, h, w, b.width, b.width, 3, b.stride)
        ho, wo = _out(h, 3, b.stride, 1), _out(w, 3, b.stride, 1)
        convs[pf + ".conv3"] = (n, ho, wo, b.width, b.cout, 1, 1)
        if b.has_ds:
            convs[pf + ".downsample.0"] = (n, h, w, b.cin, b.cout, 1, b.stride)
        h, w = ho, wo
    return convs
