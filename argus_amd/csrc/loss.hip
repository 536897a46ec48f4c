// SE(3) geodesic pose loss, forward + backward, one fused kernel.
//
// Reference: geometric_loss_fn (argus/train.py:105-119)
//     torch.sum((pp.se3(pred).Exp() @ target.Inv()).Log() ** 2, axis=-1)
// with pypose's closed forms (se3 = [rho, phi], SE3 = [t, q xyzw]):
//   Exp: q = [sin(th/2)/th phi, cos(th/2)], t = J_l(phi) rho
//   Inv: q^-1 = conj q, t^-1 = -R(q^-1) t;   Mul: (q1 q2, t1 + R(q1) t2)
//   Log: phi = 2 atan(|v|/w)/|v| v (sign-invariant), tau = J_l^-1(phi) t;  loss = |tau|^2 + |phi|^2
// The gradient is the exact derivative of this composite map (= pypose's Lie-Jacobian backward
// 2 xi^T J_l^-1(xi_r) J_l(pred)), obtained by forward-mode dual numbers over the 6 inputs. The
// per-sample arithmetic runs in fp64 (a few hundred flops per sample; the batch is <= 1024).
#include "internal.h"
#include "se3.h"

namespace argus {

ARGUS_DEV Dual se3_loss(const Dual (&xi)[6], const double (&T)[7]) {
  // Exp(pred)
  const V3 rho = {xi[0], xi[1], xi[2]};
  const V3 phi = {xi[3], xi[4], xi[5]};
  const Dual th2 = dot(phi, phi);
  const Dual th = dsqrt(th2);
  Dual imag, real;
  if (th.v < kSmall) {
    imag = cst(0.5) - (1.0 / 48) * th2 + (1.0 / 3840) * (th2 * th2);
    real = cst(1.0) - (1.0 / 8) * th2 + (1.0 / 384) * (th2 * th2);
  } else {
    imag = dsin(0.5 * th) / th;
    real = dcos(0.5 * th);
  }
  const Quat qp = {scale(imag, phi), real};
  const V3 tp = jl_apply(phi, rho, false);
  // target^-1
  const Quat qti = {{cst(-T[3]), cst(-T[4]), cst(-T[5])}, cst(T[6])};
  const V3 tt = {cst(T[0]), cst(T[1]), cst(T[2])};
  const V3 tti = scale(cst(-1.0), qrot(qti, tt));
  // Exp(pred) @ target^-1
  const Quat qr = qmul(qp, qti);
  const V3 tr = add(tp, qrot(qp, tti));
  // Log
  const Dual n2 = dot(qr.v, qr.v);
  const Dual n = dsqrt(n2);
  Dual w = qr.w;
  if (w.v == 0.0) w.v = 1e-30;
  Dual factor;
  if (n.v < kSmall) {
    factor = cst(2.0) / w - (2.0 / 3.0) * n2 / (w * w * w);
  } else {
    factor = 2.0 * datan(n / w) / n;
  }
  const V3 phr = scale(factor, qr.v);
  const V3 tau = jl_apply(phr, tr, true);
  return dot(tau, tau) + dot(phr, phr);
}

__global__ void se3_loss_kernel(int B, const float* __restrict__ pred, const float* __restrict__ target,
                                float* __restrict__ loss, float* __restrict__ dpred, float gscale) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = t / 6, dir = t - 6 * b;  // sample, input direction of this lane
  if (b >= B) return;
  Dual xi[6];
  for (int i = 0; i < 6; ++i) xi[i] = cst((double)pred[b * 6 + i]);
  xi[dir].d[0] = 1.0;
  double T[7];
  for (int i = 0; i < 7; ++i) T[i] = (double)target[b * 7 + i];
  const Dual L = se3_loss(xi, T);
  if (dir == 0) loss[b] = (float)L.v;
  if (dpred) dpred[b * 6 + dir] = (float)(gscale * L.d[0]);
}

// se(3) -> SE(3) exponential map (pypose se3.Exp): out[b] = [t (3), q xyzw (4)], w >= 0 canonical
// when `canon` (the data pipeline's quaternion convention): se3.h se3_exp_one per sample.
__global__ void se3_exp_kernel(int B, const float* __restrict__ xi, float* __restrict__ out, int canon) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  se3_exp_one(xi + b * 6, out + b * 7, canon);
}

}  // namespace argus

using namespace argus;

extern "C" int argus_se3_exp(int batch, const float* xi, float* out, int canonical_w, argus_stream_t stream) {
  if (batch <= 0 || !xi || !out) {
    set_error("se3_exp: bad arguments");
    return ARGUS_ERR_ARG;
  }
  hipLaunchKernelGGL(se3_exp_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, batch, xi, out,
                     canonical_w);
  return check_launch("se3_exp_kernel");
}

extern "C" int argus_se3_loss(int batch, const float* pred, const float* target, float* loss, float* dpred,
                              float grad_scale, argus_stream_t stream) {
  if (batch <= 0 || !pred || !target || !loss) {
    set_error("se3_loss: bad arguments");
    return ARGUS_ERR_ARG;
  }
  hipLaunchKernelGGL(se3_loss_kernel, dim3((6 * batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, batch, pred, target,
                     loss, dpred, grad_scale);
  return check_launch("se3_loss_kernel");
}
