"""int64 numpy statement of the occluder-arc definition ("Resident dataset"): which
pixels ``ImageDraw.arc((x0, y0, x1, y1), a0, a1, fill=0, width=wd)`` blackens, in the project's own
closed form. Written from the definition, not from the kernel; integers only, no float on either
side of a comparison.

An arc record is 12 int32: x0, y0, x1, y1, wd, mode, sx, sy, ex, ey, 0, 0 (source-frame pixels;
``mode`` 0 nothing / 1 full ellipse / 2 span <= 180 / 3 span > 180; (sx, sy) and (ex, ey) =
round(2^20 * (cos, sin)) of the start and end angle, clockwise from 3 o'clock, y down).

For a pixel (px, py): X = 2 px - (x0 + x1), Y = 2 py - (y0 + y1) (doubled offsets from the box centre),
A = x1 - x0 + 1, B = y1 - y0 + 1 (the diameters of the ellipse inscribed in the box of whole pixels).
  in_ell(X, Y, A, B) = A > 0 and B > 0 and X^2 B^2 + Y^2 A^2 <= A^2 B^2
  stroke  = in_ell(X, Y, A, B) and not in_ell(X, Y, A - 2 wd, B - 2 wd)
  sector(u, v): c1 = sx v - sy u >= 0, c2 = u ey - v ex >= 0; mode 1 true, 2 c1 and c2, 3 c1 or c2, 0 false
  A > 1 and B > 1:  covered = stroke and sector(X (B - 1), Y (A - 1))   (PIL's angles are parametric,
                    on the ellipse through the box's corner pixel centres: diameters A - 1, B - 1)
  A == 1 (x0 == x1, a vertical line; the one-pixel box too): the angles select the range of b sin t
  they sweep, b = B - 1:
      hi = b 2^20 if sector(0, 1) else b max(sy, ey);  lo = -b 2^20 if sector(0, -1) else b min(sy, ey)
      covered = stroke and mode != 0 and (mode == 1 or lo <= Y 2^20 <= hi)
  B == 1, A > 1 (y0 == y1, a horizontal line): lo, hi the same with a = A - 1, cos and sector(1, 0) /
  sector(-1, 0); PIL rounds the two ends to whole doubled coordinates and a pixel owns [X, X + 2):
      rl = floor((lo + 2^19) / 2^20), rh = floor((hi + 2^19) / 2^20)
      covered = stroke and mode != 0 and (mode == 1 or (X + 1 >= rl and X <= rh))
Every coordinate lies in [0, 8192): |X|, |Y| < 2^14 and A, B <= 2^13 keep every product inside int64.
A record outside that range, or with x1 < x0 or y1 < y0, covers nothing; wd is taken as clamp(wd, 1, 8192).
"""
import numpy as np

ARC_WORDS = 12
ONE = 1 << 20
FRAME = 8192


def make_record(x0, y0, x1, y1, a0, a1, wd):
    """One record from PIL's arguments (float angles allowed; wd < 1 draws as 1, as PIL does)."""
    a0, a1 = float(a0), float(a1)
    if a1 - a0 >= 360.0:
        mode, s, e = 1, 0.0, 0.0
    else:
        s, e = a0 % 360.0, a1 % 360.0
        span = (e - s) % 360.0
        mode = 0 if span == 0.0 else (2 if span <= 180.0 else 3)
    c = [int(round(ONE * f(np.deg2rad(t)))) for t in (s, e) for f in (np.cos, np.sin)]
    return np.array([x0, y0, x1, y1, max(1, int(wd)), mode, *c, 0, 0], dtype=np.int32)


def _in_ell(X, Y, A, B):
    if A <= 0 or B <= 0:
        return np.zeros(np.broadcast(X, Y).shape, dtype=bool)
    return X * X * (B * B) + Y * Y * (A * A) <= A * A * B * B


def _sector(u, v, mode, sx, sy, ex, ey):
    c1 = sx * v - sy * u >= 0
    c2 = u * ey - v * ex >= 0
    if mode == 1:
        return np.ones(np.broadcast(u, v).shape, dtype=bool)
    if mode == 2:
        return c1 & c2
    if mode == 3:
        return c1 | c2
    return np.zeros(np.broadcast(u, v).shape, dtype=bool)


def _line_range(T, D, mode, s, e, plus, minus, rounded=False):
    """Pixels of a degenerate (line) box whose doubled offset T along the line lies in the range of
    D * (cos or sin) that the angles sweep; s, e = that component of the end directions, plus / minus
    = whether the sweep contains the line's positive / negative end."""
    if mode == 0:
        return np.zeros(T.shape, dtype=bool)
    if mode == 1:
        return np.ones(T.shape, dtype=bool)
    hi = D * ONE if plus else D * max(s, e)
    lo = -D * ONE if minus else D * min(s, e)
    if rounded:  # Python's // floors, for negative numbers too
        return (T + 1 >= (lo + ONE // 2) // ONE) & (T <= (hi + ONE // 2) // ONE)
    return (T * ONE >= lo) & (T * ONE <= hi)


def arc_mask(rec, h, w, y0=0, x0=0):
    """(h, w) bool: pixels of the window at origin (y0, x0) of the source frame that ``rec`` covers."""
    bx0, by0, bx1, by1, wd, mode, sx, sy, ex, ey = (int(v) for v in np.asarray(rec).reshape(-1)[:10])
    py = (np.arange(h, dtype=np.int64) + y0)[:, None]
    px = (np.arange(w, dtype=np.int64) + x0)[None, :]
    X = np.broadcast_to(2 * px - (bx0 + bx1), (h, w))
    Y = np.broadcast_to(2 * py - (by0 + by1), (h, w))
    if not (0 <= bx0 <= bx1 < FRAME and 0 <= by0 <= by1 < FRAME and 1 <= mode <= 3):
        return np.zeros((h, w), dtype=bool)
    wd = min(max(wd, 1), FRAME)
    A, B = bx1 - bx0 + 1, by1 - by0 + 1
    stroke = _in_ell(X, Y, A, B) & ~_in_ell(X, Y, A - 2 * wd, B - 2 * wd)
    sec = lambda u, v: bool(_sector(np.int64(u), np.int64(v), mode, sx, sy, ex, ey))  # noqa: E731
    if A > 1 and B > 1:
        return stroke & _sector(X * (B - 1), Y * (A - 1), mode, sx, sy, ex, ey)
    if A == 1:
        return stroke & _line_range(Y, B - 1, mode, sy, ey, sec(0, 1), sec(0, -1))
    return stroke & _line_range(X, A - 1, mode, sx, ex, sec(1, 0), sec(-1, 0), rounded=True)


def occlude(images, arcs, y0=0, x0=0):
    """images (n_img, 3, h, w) uint8, arcs (n_img, n_arcs, 12) int32 -> copy with every covered pixel 0."""
    out = np.array(images, copy=True)
    n, _, h, w = out.shape
    for i in range(n):
        m = np.zeros((h, w), dtype=bool)
        for r in arcs[i]:
            m |= arc_mask(r, h, w, y0, x0)
        out[i][:, m] = 0
    return out
