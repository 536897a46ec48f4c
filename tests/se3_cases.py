"""The pose loss straight from the definition of the maps, and the input regimes the loss tests share.

``definition_loss`` uses none of the closed forms of ``oracle/se3.py`` (no Rodrigues coefficients, no
``J_l``, no ``atan``, no Taylor branch, no threshold): Exp is the 4x4 matrix exponential (``mp.expm``),
Log is the principal matrix logarithm (inverse scaling and squaring in mpmath arithmetic, checked per
sample; ``mp.logm`` itself returns a complex, non-principal logarithm for rotations near pi), both at
``DPS`` digits, and the gradient is a central difference at that precision. The target enters as the kernel (and the oracle) use it: its inverse
is ``(conj q, -R(conj q) t)`` with ``R(q) = I + 2 w K(v) + 2 K(v)^2`` evaluated on the *stored* q, and
the rotation of the residual is read off the *direction* of the quaternion product only (the Log
divides |v| by w), i.e. off the normalised q. For a unit q the two coincide; a stored fp32 q is unit
to 6e-8 only, and ``target_quat_scaled`` scales q on purpose.

``regimes()`` builds its inputs with the oracle's Exp / Mul: they are inputs, the reference sees
the fp32-rounded values exactly as the kernel does, and ``tests/test_oracle.py`` checks on the
definition that every sample is where its regime says (and at least 5e-4 away from a residual angle
of pi, where the principal logarithm, and so this reference, is discontinuous).

Helper of tests/test_oracle.py and tests/test_gpu_tail_kernels.py (not a test module).
"""
from __future__ import annotations

import functools
import math

import mpmath as mp
import torch

from oracle import se3

DPS = 40  # working digits of the definition (the logarithm runs at 10 more)
_H = mp.mpf(10) ** -14  # central-difference step: truncation ~ h^2 f''' and rounding ~ 10^-DPS / h, both < 1e-24


def _K(p):
    return mp.matrix([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])


def _exp_matrix(xi):
    """expm([[K(phi), rho], [0, 0]]) for xi = [rho, phi]."""
    A = mp.zeros(4)
    K = _K(xi[3:])
    for i in range(3):
        A[i, 3] = xi[i]
        for j in range(3):
            A[i, j] = K[i, j]
    return mp.expm(A)


def _quat_matrix(v, w):
    K = _K(v)
    return mp.eye(3) + 2 * w * K + 2 * K * K


def _target_inverse_matrix(T):
    t = mp.matrix(T[:3])
    v = [-T[3], -T[4], -T[5]]  # conj q
    w = T[6]
    s = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2 + w**2)
    R = _quat_matrix([c / s for c in v], w / s)  # what the Log sees: the direction of q
    ti = -(_quat_matrix(v, w) * t)  # what Inv computes: the stored q
    M = mp.eye(4)
    for i in range(3):
        M[i, 3] = ti[i]
        for j in range(3):
            M[i, j] = R[i, j]
    return M


def _affine_inverse(A):
    """Inverse of [[R, t], [0, 1]] = [[R^-1, -R^-1 t], [0, 1]], R^-1 by the adjugate (every matrix the
    logarithm below inverts has this form; ``mp.inverse`` gives the same at several times the cost)."""
    assert A.rows == 4 and A[3, 0] == 0 and A[3, 1] == 0 and A[3, 2] == 0 and A[3, 3] == 1
    (a, b, c), (d, e, f), (g, h, i) = [[A[r, 0], A[r, 1], A[r, 2]] for r in range(3)]
    co = [[e * i - f * h, c * h - b * i, b * f - c * e],
          [f * g - d * i, a * i - c * g, c * d - a * f],
          [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * co[0][0] + b * co[1][0] + c * co[2][0]
    out = mp.eye(4)
    for r in range(3):
        for k in range(3):
            out[r, k] = co[r][k] / det
        out[r, 3] = -sum(co[r][k] * A[k, 3] for k in range(3)) / det
    return out


def _principal_logm(M):
    """Principal logarithm of a real affine 4x4 matrix without eigenvalues on the closed negative axis: inverse
    scaling and squaring, log M = 2^k log M^(1/2^k), each principal square root by the plain Denman-Beavers
    iteration and the last logarithm by the Mercator series. All in real arithmetic, so the result is a
    real logarithm. (``mp.logm`` is not principal here: its ``sqrtm`` switches to a complex-rotated,
    non-principal root once the iteration needs more than six steps, which a rotation within ~0.1 of pi
    does. ``_loss`` checks the result instead of trusting either.)"""
    I = mp.eye(M.rows)
    tol = mp.eps * 64
    B, k = M, 0
    while mp.mnorm(B - I, "inf") >= 0.125:
        Y, Z = B, I
        for _ in range(200):
            Y, Z, prev = (Y + _affine_inverse(Z)) / 2, (Z + _affine_inverse(Y)) / 2, Y
            if mp.mnorm(Y - prev, "inf") <= tol * mp.mnorm(Y, "inf"):
                break
        else:
            raise mp.NoConvergence("sqrtm")
        B, k = Y, k + 1
    X = B - I
    L, P, j = X * 0, X, 1
    while mp.mnorm(P, "inf") >= tol:
        L += P / j if j & 1 else -P / j
        P, j = P * X, j + 1
    return L * 2**k


def _loss(xi, Tinv, check=False):
    M = _exp_matrix(xi) * Tinv
    with mp.extradps(10):
        L = _principal_logm(M)
        if check:  # a real logarithm of M with rotation angle < pi is the principal one
            assert mp.mnorm(mp.expm(L) - M, "inf") < mp.mpf(10) ** (5 - DPS) * mp.mnorm(M, "inf")
            assert (L[2, 1] ** 2 + L[0, 2] ** 2 + L[1, 0] ** 2) < mp.pi**2
    phi = [(L[2, 1] - L[1, 2]) / 2, (L[0, 2] - L[2, 0]) / 2, (L[1, 0] - L[0, 1]) / 2]
    val = sum(L[i, 3] ** 2 for i in range(3)) + sum(c**2 for c in phi)
    return val, mp.sqrt(sum(c**2 for c in phi))


def definition_loss(pred: torch.Tensor, target: torch.Tensor):
    """(loss (n,), d loss / d pred (n, 6), residual angle (n,)) as fp64 tensors, computed at DPS digits
    from the fp32 values of ``pred`` (n, 6) and ``target`` (n, 7)."""
    assert pred.dtype == torch.float32 and target.dtype == torch.float32
    losses, grads, angles = [], [], []
    with mp.workdps(DPS):
        for p, T in zip(pred.tolist(), target.tolist()):
            xi = [mp.mpf(c) for c in p]
            Tinv = _target_inverse_matrix([mp.mpf(c) for c in T])
            val, ang = _loss(xi, Tinv, check=True)
            g = []
            for i in range(6):
                hi = list(xi)
                lo = list(xi)
                hi[i] += _H
                lo[i] -= _H
                g.append(float((_loss(hi, Tinv)[0] - _loss(lo, Tinv)[0]) / (2 * _H)))
            losses.append(float(val))
            grads.append(g)
            angles.append(float(ang))
    return (torch.tensor(losses, dtype=torch.float64), torch.tensor(grads, dtype=torch.float64),
            torch.tensor(angles, dtype=torch.float64))


def definition_exp(xi: torch.Tensor) -> torch.Tensor:
    """Exp of fp32 se(3) vectors (n, 6) as fp64 [t, q xyzw] (n, 7), q not sign-canonicalised: t is the last
    column of the 4x4 matrix exponential, q the SU(2) exponential expm(-i/2 phi . sigma) = w - i (v . sigma)."""
    assert xi.dtype == torch.float32
    out = []
    with mp.workdps(DPS):
        for p in xi.tolist():
            x = [mp.mpf(c) for c in p]
            E = _exp_matrix(x)
            a, b, c = x[3], x[4], x[5]
            U = mp.expm(mp.mpc(0, -0.5) * mp.matrix([[c, mp.mpc(a, -b)], [mp.mpc(a, b), -c]]))
            out.append([float(E[0, 3]), float(E[1, 3]), float(E[2, 3]),
                        float(-mp.im(U[1, 0])), float(mp.re(U[1, 0])), float(-mp.im(U[0, 0])), float(mp.re(U[0, 0]))])
    return torch.tensor(out, dtype=torch.float64)


def _unit(n, g):
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def _target_for_residual(pred32, delta):
    """fp32 target T with Exp(pred) @ T^-1 = Exp(delta) (up to the fp32 rounding of T)."""
    return se3.se3_mul(se3.se3_exp(-delta), se3.se3_exp(pred32.double())).float()


@functools.lru_cache(maxsize=None)
def regimes():
    """name -> (pred fp32 (n, 6), target fp32 (n, 7)); fixed seeds, n <= 32. Treat as read-only."""
    out = {}
    g = torch.Generator().manual_seed(1201)
    out["generic"] = (torch.randn(6, 6, generator=g).float(), se3.random_targets(6, generator=g, sigma=1.0))

    # |phi| on both sides of the 1e-4 Taylor threshold of Exp and J_l
    g = torch.Generator().manual_seed(1202)
    ang = torch.tensor([0.0, 1e-7, 0.99e-4, 1.01e-4, 1e-3], dtype=torch.float64).repeat_interleave(2)
    pred = torch.cat([torch.randn(10, 3, generator=g, dtype=torch.float64), ang[:, None] * _unit(10, g)], -1).float()
    out["pred_small_angle"] = (pred, se3.random_targets(10, generator=g, sigma=0.5))

    # residual angle theta: n = sin(theta / 2) crosses the Log's 1e-4 threshold at theta = 2e-4
    g = torch.Generator().manual_seed(1203)
    th = torch.tensor([0.0, 1e-6, 1.98e-4, 2.02e-4, 1e-3], dtype=torch.float64).repeat_interleave(2)
    pred = (torch.randn(10, 6, generator=g) * 0.8).float()
    scale = th.clamp_min(1e-7)[:, None]  # residual translation of the size of the residual angle
    delta = torch.cat([scale * torch.randn(10, 3, generator=g, dtype=torch.float64), th[:, None] * _unit(10, g)], -1)
    out["residual_small"] = (pred, _target_for_residual(pred, delta))

    # residual angle near pi from both sides; pi + d lands on the w < 0 side of the Log
    g = torch.Generator().manual_seed(1204)
    th = (math.pi + torch.tensor([-1e-2, -1e-3, 1e-3, 1e-2], dtype=torch.float64)).repeat_interleave(2)
    pred = (torch.randn(8, 6, generator=g) * 0.8).float()
    delta = torch.cat([torch.randn(8, 3, generator=g, dtype=torch.float64), th[:, None] * _unit(8, g)], -1)
    out["residual_near_pi"] = (pred, _target_for_residual(pred, delta))

    # |phi| beyond pi and around 2 pi: w of Exp(pred) is negative; against near-identity targets the
    # residual has w ~ -1. The last four samples rotate the target about the prediction's own axis so that
    # the residual angle is 2 pi +- 5e-5: the Taylor branch of the Log (n = 2.5e-5) with w < 0.
    g = torch.Generator().manual_seed(1205)
    ang = torch.tensor([4.0, 2 * math.pi - 1e-3, 2 * math.pi + 1e-3, 7.5], dtype=torch.float64).repeat_interleave(2)
    pred = torch.cat([torch.randn(8, 3, generator=g, dtype=torch.float64), ang[:, None] * _unit(8, g)], -1).float()
    near = se3.random_targets(8, generator=g, sigma=1e-3)
    far = se3.random_targets(8, generator=g, sigma=1.0)
    T = torch.where((torch.arange(8) % 2 == 0)[:, None], near, far)
    d = torch.tensor([-1e-3, -1e-3, 1e-3, 1e-3], dtype=torch.float64)
    e = torch.tensor([5e-5, -5e-5, 5e-5, -5e-5], dtype=torch.float64)
    axis = _unit(4, g)
    pred2 = torch.cat([torch.randn(4, 3, generator=g, dtype=torch.float64), (2 * math.pi + d)[:, None] * axis], -1).float()
    xi_t = torch.cat([1e-3 * torch.randn(4, 3, generator=g, dtype=torch.float64), (d - e)[:, None] * axis], -1)
    out["pred_beyond_pi"] = (torch.cat([pred, pred2]), torch.cat([T, se3.se3_exp(xi_t).float()]))

    g = torch.Generator().manual_seed(1206)
    s = torch.tensor([100.0, 100.0, 100.0, 0.5, 0.5, 0.5], dtype=torch.float64)
    pred = (torch.randn(4, 6, generator=g, dtype=torch.float64) * s).float()
    out["large_translation"] = (pred, se3.se3_exp(torch.randn(4, 6, generator=g, dtype=torch.float64) * s).float())

    # the Log reads only the direction of the residual quaternion, on either branch: targets whose q is
    # scaled by s (s < 0: the other cover). With |s| != 1 the Taylor branch (n = |s| sin(theta / 2) < 1e-4)
    # runs with a w that is not +-1, which is what tells `2 / w` from `2`: with a unit q the loss and its
    # gradient are even in the residual rotation vector and blind to the sign of that factor.
    # Pure-rotation targets (t = 0), prediction translation of the size of the residual angle.
    g = torch.Generator().manual_seed(1207)
    th = torch.tensor([2e-5, 8e-5, 1e-3, 1.0], dtype=torch.float64).repeat_interleave(3)
    s = torch.tensor([0.5, 2.0, -1.0, -0.5, 0.5, 2.0, 2.0, -0.5, 0.5, 0.5, 2.0, -1.0], dtype=torch.float64)
    phi = (torch.randn(12, 3, generator=g) * 0.8).float()
    pred = torch.cat([torch.zeros(12, 3), phi], -1)
    delta = torch.cat([torch.zeros(12, 3, dtype=torch.float64), th[:, None] * _unit(12, g)], -1)
    q = _target_for_residual(pred, delta)[:, 3:].double() * s[:, None]
    rho = th[:, None] * torch.randn(12, 3, generator=g, dtype=torch.float64)
    out["target_quat_scaled"] = (torch.cat([rho.float(), phi], -1), torch.cat([torch.zeros(12, 3), q.float()], -1))
    for p, T in out.values():
        assert p.dtype == T.dtype == torch.float32 and p.shape[0] == T.shape[0] <= 32
    return out


EXP_REGIMES = ("pred_small_angle", "pred_beyond_pi", "generic")

# Per-sample bars of oracle/se3.py against the definition: |d loss| <= r_loss |loss| + a_loss and
# |d grad|_inf <= r_grad |grad|_inf + a_grad. Each constant is 4x the worst discrepancy measured on the
# development CPU (torch fp64 oracle against definition_loss, these seeds): the relative one over the
# samples with |loss| (|grad|_inf) >= 1e-3, the absolute one over the samples below 1e-3, where the fp64
# cancellation in the quaternion product and in t_pred - R t_target sets an absolute floor. Measured:
#   regime              rel loss  abs loss  rel grad  abs grad
#   generic             3.2e-16   -         5.4e-16   -
#   pred_small_angle    1.0e-13   -         1.9e-09   -        (Taylor truncation / (1 - cos th) / th^2 at th ~ 1e-4)
#   residual_small      -         2.4e-19   1.7e-13   1.4e-15
#   residual_near_pi    3.4e-16   -         8.4e-16   -
#   pred_beyond_pi      5.9e-16   -         5.7e-14   -
#   large_translation   4.0e-16   -         7.1e-15   -
#   target_quat_scaled  1.9e-16   8.8e-20   9.7e-14   3.4e-16
# ("-": the regime has no sample on that side of 1e-3.) The GPU tests add a_loss / a_grad to the kernel's bar.
SMALL = 1e-3
BARS = {
    "generic": dict(r_loss=4 * 3.2e-16, a_loss=0.0, r_grad=4 * 5.4e-16, a_grad=0.0),
    "pred_small_angle": dict(r_loss=4 * 1.0e-13, a_loss=0.0, r_grad=4 * 1.9e-9, a_grad=0.0),
    "residual_small": dict(r_loss=0.0, a_loss=4 * 2.4e-19, r_grad=4 * 1.7e-13, a_grad=4 * 1.4e-15),
    "residual_near_pi": dict(r_loss=4 * 3.4e-16, a_loss=0.0, r_grad=4 * 8.4e-16, a_grad=0.0),
    "pred_beyond_pi": dict(r_loss=4 * 5.9e-16, a_loss=0.0, r_grad=4 * 5.7e-14, a_grad=0.0),
    "large_translation": dict(r_loss=4 * 4.0e-16, a_loss=0.0, r_grad=4 * 7.1e-15, a_grad=0.0),
    "target_quat_scaled": dict(r_loss=4 * 1.9e-16, a_loss=4 * 8.8e-20, r_grad=4 * 9.7e-14, a_grad=4 * 3.4e-16),
}

# se3.se3_exp against definition_exp, same kind of bar: |d t|_inf <= r_t max(1, |t|_inf), |d q|_inf <= a_q.
# Measured (r_t, a_q): pred_small_angle (1.6e-13, 5.4e-20), pred_beyond_pi (3.3e-16, 2.3e-16),
# generic (2.0e-16, 1.2e-16).
EXP_BARS = {
    "pred_small_angle": dict(r_t=4 * 1.6e-13, a_q=4 * 5.4e-20),
    "pred_beyond_pi": dict(r_t=4 * 3.3e-16, a_q=4 * 2.3e-16),
    "generic": dict(r_t=4 * 2.0e-16, a_q=4 * 1.2e-16),
}


@functools.lru_cache(maxsize=None)
def definition_results(name: str):
    """definition_loss on a regime, computed once per process."""
    return definition_loss(*regimes()[name])
