// ani_kernels_md_nh.hip — Nose-Hoover chain, isotropic barostat and thermo record of the timestep loop (include/ani_md.h,
// ani_md_nh_*, ani_md_npt_*, ani_md_thermo): one unit, they share the chain's half-step and the kinetic sums
#include "ani_md_device.h"

namespace {

// ---- Nose-Hoover chain and thermo record (include/ani_md.h, ani_md_nh_* / ani_md_thermo) ------------------------------------
// Sums as FIRE's: per-block partials with block_sum_fixed, then one workgroup that strides over the partials and sums its 256
// accumulators with block_sum_fixed again.  The chain itself is a few dozen flops on one thread.
constexpr double NH_BOLTZ = 0.0019872067, NH_MVV2E = 48.88821291 * 48.88821291, NH_NKTV2P = 68568.415;

// m |v|^2 mvv2e of one atom, the multiply-adds spelled out: the same bits wherever it is inlined
__device__ __forceinline__ double k2_term(double m, double v0, double v1, double v2) {
  return (m * fma(v2, v2, fma(v1, v1, v0 * v0))) * NH_MVV2E;
}

__global__ __launch_bounds__(256) void nh_kinetic_kernel(const double* __restrict__ v, const double* __restrict__ mass, int n,
                                                         double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double k2 = 0.0;
  if (i < n) k2 = k2_term(mass[i], v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]);
  k2 = block_sum_fixed(k2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = k2;
}

// The chain's half-step of include/ani_md.h on one thread: K2 is scaled in place, s and ecouple come back, eta / ed / edd are the
// chain's links in registers (chain_load / the caller's stores).  The thermostat chain and the barostat chain are this one function.
// kt = k_B t_target and ket = tdof kt come rounded from the host: formed here, K2 - tdof kt would contract into one multiply-add
// and a chain at rest exactly on target would start to move.
static_assert(ANI_MD_NH_ETA_DOT - ANI_MD_NH_ETA == ANI_MD_NH_MAXCHAIN && ANI_MD_NH_ETA_DOTDOT - ANI_MD_NH_ETA_DOT == ANI_MD_NH_MAXCHAIN &&
              ANI_MD_NPT_ETA_DOT - ANI_MD_NPT_ETA == ANI_MD_NH_MAXCHAIN && ANI_MD_NPT_ETA_DOTDOT - ANI_MD_NPT_ETA_DOT == ANI_MD_NH_MAXCHAIN,
              "chain_load reads eta, eta_dot and eta_dotdot of either record as three blocks behind one another");
__device__ __forceinline__ void chain_load(const double* __restrict__ links, int M, double (&eta)[ANI_MD_NH_MAXCHAIN],
                                           double (&ed)[ANI_MD_NH_MAXCHAIN + 1], double (&edd)[ANI_MD_NH_MAXCHAIN]) {
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) {
    const bool used = k < M;
    eta[k] = used ? links[k] : 0.0;
    ed[k] = used ? links[ANI_MD_NH_MAXCHAIN + k] : 0.0;
    edd[k] = used ? links[2 * ANI_MD_NH_MAXCHAIN + k] : 0.0;
  }
  ed[ANI_MD_NH_MAXCHAIN] = 0.0;
}
__device__ __forceinline__ void chain_half_step(double& K2, double kt, double ket, double t_period, double drag, double dt, int M,
                                                int nc, double (&eta)[ANI_MD_NH_MAXCHAIN], double (&ed)[ANI_MD_NH_MAXCHAIN + 1],
                                                double (&edd)[ANI_MD_NH_MAXCHAIN], double& s_out, double& ec_out) {
  double Q[ANI_MD_NH_MAXCHAIN];
  const double tf = 1.0 / t_period;
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) Q[k] = (k == 0 ? ket : kt) / (tf * tf);
  const double nf = 1.0 / (double)nc, dfac = 1.0 - dt * drag / (double)nc;
  const double h2 = nf * dt / 2.0, h4 = nf * dt / 4.0, h8 = nf * dt / 8.0;
  edd[0] = (K2 - ket) / Q[0];
  double s = 1.0;
  for (int it = 0; it < nc; it++) {
    for (int k = M - 1; k >= 1; k--) {
      const double e = exp(-h8 * ed[k + 1]);
      ed[k] = ((ed[k] * e + edd[k] * h4) * dfac) * e;
    }
    const double e0 = exp(-h8 * ed[1]);
    ed[0] = ((ed[0] * e0 + edd[0] * h4) * dfac) * e0;
    const double fac = exp(-h2 * ed[0]);
    s *= fac;
    K2 *= fac * fac;
    edd[0] = (K2 - ket) / Q[0];
    for (int k = 0; k < M; k++) eta[k] += h2 * ed[k];
    ed[0] = (ed[0] * e0 + edd[0] * h4) * e0;
    for (int k = 1; k < M; k++) {
      const double e = exp(-h8 * ed[k + 1]);
      ed[k] *= e;
      edd[k] = (Q[k - 1] * ed[k - 1] * ed[k - 1] - kt) / Q[k];
      ed[k] = (ed[k] + edd[k] * h4) * e;
    }
  }
  double ec = ket * eta[0] + 0.5 * Q[0] * ed[0] * ed[0];
  for (int k = 1; k < M; k++) ec += kt * eta[k] + 0.5 * Q[k] * ed[k] * ed[k];
  s_out = s;
  ec_out = ec;
}

__global__ __launch_bounds__(256) void nh_chain_kernel(double* __restrict__ state, const double* __restrict__ part, int npart,
                                                       double t_target, double tdof, double kt, double ket,
                                                       ani_md_nh_params p) {
  __shared__ double red[4];
  double K2 = 0.0;
  for (int b = threadIdx.x; b < npart; b += 256) K2 += part[b];
  K2 = block_sum_fixed(K2, red);
  if (threadIdx.x != 0) return;
  if (npart == 0) K2 = state[ANI_MD_NH_K2];
  state[ANI_MD_NH_T_TARGET] = t_target;
  state[ANI_MD_NH_TDOF] = tdof;
  state[ANI_MD_NH_ZERO] = 0.0;
  if (!finite_d(K2)) {
    state[ANI_MD_NH_K2] = K2;
    state[ANI_MD_NH_S] = 1.0;
    state[ANI_MD_NH_NONFINITE] += 1.0;
    return;
  }
  double eta[ANI_MD_NH_MAXCHAIN], ed[ANI_MD_NH_MAXCHAIN + 1], edd[ANI_MD_NH_MAXCHAIN];
  chain_load(state + ANI_MD_NH_ETA, p.mtchain, eta, ed, edd);
  double s, ec;
  chain_half_step(K2, kt, ket, p.t_period, p.drag, p.dt, p.mtchain, p.nc_tchain, eta, ed, edd, s, ec);
  state[ANI_MD_NH_HALF_STEPS] += 1.0;
  state[ANI_MD_NH_K2] = K2;
  state[ANI_MD_NH_S] = s;
  state[ANI_MD_NH_ECOUPLE] = ec;
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) {
    state[ANI_MD_NH_ETA + k] = eta[k];
    state[ANI_MD_NH_ETA_DOT + k] = ed[k];
    state[ANI_MD_NH_ETA_DOTDOT + k] = edd[k];
  }
}

__global__ __launch_bounds__(256) void nh_scale_kernel(double* __restrict__ v, int n, const double* __restrict__ state) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < 3 * n) v[t] *= state[ANI_MD_NH_S];
}

// initial_integrate_kernel with v = s v in front of it
__global__ __launch_bounds__(256) void nh_initial_integrate_kernel(double* __restrict__ x, double* __restrict__ v,
                                                                   const double* __restrict__ f, const double* __restrict__ dtfm,
                                                                   double dt, int n, const double* __restrict__ xb,
                                                                   double* __restrict__ d2max, const double* __restrict__ state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double d2 = 0.0;
  if (i < n) {
    const double s = dtfm[i], sc = state[ANI_MD_NH_S];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double vk = fma(s, f[3 * i + k], sc * v[3 * i + k]);   // s v rounded, then the kick as initial_integrate_kernel contracts it
      d2 += drift_d2(x, v, xb, 3 * i + k, dt, vk);
    }
  }
  __shared__ double red[4];
  d2 = block_max(d2, red);
  if (threadIdx.x == 0) raise_d2max(d2, d2max);
}

// final_integrate_kernel without the thermostat term, and nh_kinetic_kernel on what it wrote
__global__ __launch_bounds__(256) void nh_final_integrate_kernel(double* __restrict__ v, const double* __restrict__ f,
                                                                 const double* __restrict__ dtfm, const double* __restrict__ mass,
                                                                 int n, double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double k2 = 0.0;
  if (i < n) {
    const double s = dtfm[i];
    double vn[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      vn[k] = v[3 * (size_t)i + k] + s * f[3 * (size_t)i + k];
      v[3 * (size_t)i + k] = vn[k];
    }
    k2 = k2_term(mass[i], vn[0], vn[1], vn[2]);
  }
  k2 = block_sum_fixed(k2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = k2;
}

// ---- isotropic barostat (include/ani_md.h, ani_md_npt_*) --------------------------------------------------------------------
// The box is six doubles of the barostat record; one thread of one workgroup moves it, the per-atom kernels read mu, fv, c and the
// shift ratio from the record.  Everything a half-step decides is formed in registers first and written only when K2, Wtr and the
// new strain rate are finite.

__global__ void npt_init_kernel(double* __restrict__ ps, double lo0, double lo1, double lo2, double l0, double l1, double l2, double n) {
  for (int k = 0; k < ANI_MD_NPT_NSTATE; k++) ps[k] = 0.0;
  const double lo[3] = {lo0, lo1, lo2}, len[3] = {l0, l1, l2};
  for (int k = 0; k < 3; k++) {
    ps[ANI_MD_NPT_LO + k] = lo[k];
    ps[ANI_MD_NPT_LEN + k] = len[k];
    ps[ANI_MD_NPT_RATIO + k] = 1.0;
    ps[ANI_MD_NPT_C + k] = lo[k] + 0.5 * len[k];
  }
  const double V = (l0 * l1) * l2;
  ps[ANI_MD_NPT_FV] = 1.0;
  ps[ANI_MD_NPT_MU] = 1.0;
  ps[ANI_MD_NPT_V0] = V;
  ps[ANI_MD_NPT_VOL] = V;
  ps[ANI_MD_NPT_NATOMS] = n;
}

__global__ __launch_bounds__(256) void npt_chain_kernel(int phase, double* __restrict__ ns, double* __restrict__ ps,
                                                        const double* __restrict__ part, int npart, const double* __restrict__ ev,
                                                        double t_target, double p_target, double tdof, double kt, double ket,
                                                        ani_md_npt_params p) {
  __shared__ double red[4];
  double K2 = 0.0;
  for (int b = threadIdx.x; b < npart; b += 256) K2 += part[b];
  K2 = block_sum_fixed(K2, red);
  if (threadIdx.x != 0) return;
  if (npart == 0) K2 = ns[ANI_MD_NH_K2];
  const double K2_in = K2;
  const double Wtr = (ev[1] + ev[5]) + ev[9];
  const double N = ps[ANI_MD_NPT_NATOMS];
  const double W = ((N + 1.0) * kt) * (p.p_period * p.p_period);
  double lo[3], len[3], c[3];
  for (int k = 0; k < 3; k++) { lo[k] = ps[ANI_MD_NPT_LO + k]; len[k] = ps[ANI_MD_NPT_LEN + k]; c[k] = ps[ANI_MD_NPT_C + k]; }
  const double V = (len[0] * len[1]) * len[2];
  double wd = ps[ANI_MD_NPT_OMEGA_DOT];
  double eta[ANI_MD_NH_MAXCHAIN], ed[ANI_MD_NH_MAXCHAIN + 1], edd[ANI_MD_NH_MAXCHAIN];
  double peta[ANI_MD_NH_MAXCHAIN], ped[ANI_MD_NH_MAXCHAIN + 1], pedd[ANI_MD_NH_MAXCHAIN];
  chain_load(ns + ANI_MD_NH_ETA, p.mtchain, eta, ed, edd);
  chain_load(ps + ANI_MD_NPT_ETA, p.mpchain, peta, ped, pedd);
  double s = 1.0, ec = 0.0, sb = 1.0, ecb = 0.0, P = 0.0;
  const double hdt = 0.5 * p.dt;
  if (phase == 0) {
    double Kb = (W * wd) * wd;
    chain_half_step(Kb, kt, kt, p.p_period, 0.0, p.dt, p.mpchain, p.nc_pchain, peta, ped, pedd, sb, ecb);
    wd *= sb;
    chain_half_step(K2, kt, ket, p.t_period, p.drag, p.dt, p.mtchain, p.nc_tchain, eta, ed, edd, s, ec);
  }
  {
    P = (K2 + Wtr) / (3.0 * V) * NH_NKTV2P;
    const double a = (P - p_target) * V / NH_NKTV2P, b = K2 / (3.0 * N);
    wd += hdt * ((a + b) / W);
  }
  if (phase != 0) {
    chain_half_step(K2, kt, ket, p.t_period, p.drag, p.dt, p.mtchain, p.nc_tchain, eta, ed, edd, s, ec);
    double Kb = (W * wd) * wd;
    chain_half_step(Kb, kt, kt, p.p_period, 0.0, p.dt, p.mpchain, p.nc_pchain, peta, ped, pedd, sb, ecb);
    wd *= sb;
  }
  ns[ANI_MD_NH_T_TARGET] = t_target;
  ns[ANI_MD_NH_TDOF] = tdof;
  ns[ANI_MD_NH_ZERO] = 0.0;
  ps[ANI_MD_NPT_P_TARGET] = p_target;
  if (!(finite_d(K2_in) && finite_d(Wtr) && finite_d(wd))) {
    ns[ANI_MD_NH_K2] = K2_in;
    ns[ANI_MD_NH_S] = 1.0;
    ns[ANI_MD_NH_NONFINITE] += 1.0;
    ps[ANI_MD_NPT_FV] = 1.0;
    ps[ANI_MD_NPT_MU] = 1.0;
    for (int k = 0; k < 3; k++) ps[ANI_MD_NPT_RATIO + k] = 1.0;
    ps[ANI_MD_NPT_NONFINITE] += 1.0;
    return;
  }
  double Vnew = V;
  if (phase == 0) {
    const double fv = exp(-hdt * (wd * (1.0 + 1.0 / N))), mu = exp(hdt * wd), mu2 = mu * mu;
    ps[ANI_MD_NPT_FV] = fv;
    ps[ANI_MD_NPT_MU] = mu;
    double ln[3];
    for (int k = 0; k < 3; k++) {
      ln[k] = len[k] * mu2;
      const double d = lo[k] - c[k];
      ps[ANI_MD_NPT_LO + k] = c[k] + mu2 * d;
      ps[ANI_MD_NPT_LEN + k] = ln[k];
      ps[ANI_MD_NPT_RATIO + k] = ln[k] / len[k];
    }
    Vnew = (ln[0] * ln[1]) * ln[2];
    ps[ANI_MD_NPT_OMEGA] += p.dt * wd;
  }
  ns[ANI_MD_NH_HALF_STEPS] += 1.0;
  ns[ANI_MD_NH_K2] = K2;
  ns[ANI_MD_NH_S] = s;
  ns[ANI_MD_NH_ECOUPLE] = ec;
  ps[ANI_MD_NPT_HALF_STEPS] += 1.0;
  ps[ANI_MD_NPT_OMEGA_DOT] = wd;
  ps[ANI_MD_NPT_PRESS] = P;
  ps[ANI_MD_NPT_W] = W;
  ps[ANI_MD_NPT_VOL] = Vnew;
  ps[ANI_MD_NPT_ECOUPLE_CHAIN] = ecb;
  ps[ANI_MD_NPT_ECOUPLE] = 3.0 * (0.5 * W * wd * wd + ecb) + p_target * (Vnew - ps[ANI_MD_NPT_V0]) / NH_NKTV2P;
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) {
    ns[ANI_MD_NH_ETA + k] = eta[k];
    ns[ANI_MD_NH_ETA_DOT + k] = ed[k];
    ns[ANI_MD_NH_ETA_DOTDOT + k] = edd[k];
    ps[ANI_MD_NPT_ETA + k] = peta[k];
    ps[ANI_MD_NPT_ETA_DOT + k] = ped[k];
    ps[ANI_MD_NPT_ETA_DOTDOT + k] = pedd[k];
  }
}

// step 5 of the first half on the owned rows, step 7 on the shift rows behind them: one grid over n + nghost rows
__global__ __launch_bounds__(256) void npt_initial_integrate_kernel(double* __restrict__ x, double* __restrict__ v,
                                                                    const double* __restrict__ f, const double* __restrict__ dtfm,
                                                                    double dt, int n, const double* __restrict__ xb,
                                                                    double* __restrict__ d2max, const double* __restrict__ ns,
                                                                    const double* __restrict__ ps, double* __restrict__ shift,
                                                                    int nghost) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double d2 = 0.0;
  if (i < n) {
    const double s = dtfm[i], sc = ns[ANI_MD_NH_S] * ps[ANI_MD_NPT_FV], mu = ps[ANI_MD_NPT_MU];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const size_t e = 3 * (size_t)i + k;
      const double c = ps[ANI_MD_NPT_C + k];
      const double vk = sc * v[e] + s * f[e];
      double xk = c + mu * (x[e] - c);
      xk = xk + dt * vk;
      xk = c + mu * (xk - c);
      v[e] = vk;
      x[e] = xk;
      const double d = xk - xb[e];
      d2 += d * d;
    }
  } else if (i - n < nghost) {
    const size_t g = 3 * (size_t)(i - n);
#pragma unroll
    for (int k = 0; k < 3; k++) shift[g + k] *= ps[ANI_MD_NPT_RATIO + k];
  }
  __shared__ double red[4];
  d2 = block_max(d2, red);
  if (threadIdx.x == 0 && blockIdx.x * blockDim.x < n) raise_d2max(d2, d2max);
}

// nh_final_integrate_kernel with v *= fv behind the kick; the partials are nh_kinetic_kernel's on what it wrote
__global__ __launch_bounds__(256) void npt_final_integrate_kernel(double* __restrict__ v, const double* __restrict__ f,
                                                                  const double* __restrict__ dtfm, const double* __restrict__ mass,
                                                                  int n, const double* __restrict__ ps, double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double k2 = 0.0;
  if (i < n) {
    const double s = dtfm[i], fv = ps[ANI_MD_NPT_FV];
    double vn[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      vn[k] = (v[3 * (size_t)i + k] + s * f[3 * (size_t)i + k]) * fv;
      v[3 * (size_t)i + k] = vn[k];
    }
    k2 = k2_term(mass[i], vn[0], vn[1], vn[2]);
  }
  k2 = block_sum_fixed(k2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = k2;
}

__global__ void npt_check_kernel(double* __restrict__ d2max, const double* __restrict__ ev, const double* __restrict__ ps,
                                 double* __restrict__ out) {
  const double e = ev[0];
  out[0] = finite_d(e) ? d2max[0] : __longlong_as_double(0x7ff0000000000000LL);
  d2max[0] = 0.0;
  for (int k = 0; k < ANI_MD_NPT_NSTATE; k++) out[1 + k] = ps[k];
}

// part[c nblk + b] = K_c of block b, c = xx, yy, zz, xy, xz, yz
__global__ __launch_bounds__(256) void thermo_reduce_kernel(const double* __restrict__ v, const double* __restrict__ mass, int n,
                                                            double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x, nblk = gridDim.x;
  double k[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const double m = mass[i], v0 = v[3 * (size_t)i], v1 = v[3 * (size_t)i + 1], v2 = v[3 * (size_t)i + 2];
    k[0] = (m * v0 * v0) * NH_MVV2E; k[1] = (m * v1 * v1) * NH_MVV2E; k[2] = (m * v2 * v2) * NH_MVV2E;
    k[3] = (m * v0 * v1) * NH_MVV2E; k[4] = (m * v0 * v2) * NH_MVV2E; k[5] = (m * v1 * v2) * NH_MVV2E;
  }
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const double sum = block_sum_fixed(k[c], red);
    if (threadIdx.x == 0) part[c * nblk + blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(256) void thermo_finish_kernel(const double* __restrict__ part, int nblk, const double* __restrict__ ev,
                                                            int with_virial, double tdof, double volume,
                                                            const double* __restrict__ nh_state, double* __restrict__ out) {
  __shared__ double red[4];
  double K[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) a += part[c * nblk + b];
    K[c] = block_sum_fixed(a, red);
  }
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double k2 = (K[0] + K[1]) + K[2], ke = 0.5 * k2, pe = ev[0];
  const double ec = nh_state ? nh_state[ANI_MD_NH_ECOUPLE] : 0.0;
  out[ANI_MD_THERMO_PE] = pe;
  out[ANI_MD_THERMO_KE] = ke;
  out[ANI_MD_THERMO_TEMP] = 2.0 * ke / (tdof * NH_BOLTZ);
  // W_ab = ev[1 + 3 a + b]: xx, yy, zz at 1, 5, 9; xy, xz, yz at 2, 3, 6
  const int wi[6] = {1, 5, 9, 2, 3, 6};
  out[ANI_MD_THERMO_PRESS] = with_virial ? (k2 + ((ev[1] + ev[5]) + ev[9])) / (3.0 * volume) * NH_NKTV2P : nan;
#pragma unroll
  for (int c = 0; c < 6; c++) out[ANI_MD_THERMO_PXX + c] = with_virial ? (K[c] + ev[wi[c]]) / volume * NH_NKTV2P : nan;
  out[ANI_MD_THERMO_ETOTAL] = pe + ke;
  out[ANI_MD_THERMO_ECOUPLE] = ec;
  out[ANI_MD_THERMO_ECONSERVE] = (pe + ke) + ec;
  out[ANI_MD_THERMO_VOL] = volume;
  out[ANI_MD_THERMO_K2] = k2;
  out[ANI_MD_THERMO_ZERO] = 0.0;
}

}  // namespace

extern "C" {

int ani_md_nh_work_size(int nlocal) { return nblocks(nlocal); }

int ani_md_nh_init(double* state, void* stream) {
  if (!state) return (int)hipErrorInvalidValue;
  return (int)hipMemsetAsync(state, 0, sizeof(double) * ANI_MD_NH_NSTATE, (hipStream_t)stream);
}

int ani_md_nh_kinetic(const double* v, const double* mass, int nlocal, double* work, void* stream) {
  if (nlocal <= 0) return 0;
  if (!v || !mass || !work) return (int)hipErrorInvalidValue;
  return launch(nh_kinetic_kernel, blocks(nlocal), 256, stream, v, mass, nlocal, work);
}

int ani_md_nh_chain(double* state, const double* work, int npart, double t_target, double tdof, const ani_md_nh_params* params,
                    void* stream) {
  if (!state || !params || npart < 0 || (npart > 0 && !work)) return (int)hipErrorInvalidValue;
  if (params->mtchain < 1 || params->mtchain > ANI_MD_NH_MAXCHAIN || params->nc_tchain < 1 || !(params->t_period > 0.0) ||
      !(params->dt > 0.0) || !(t_target > 0.0) || !(tdof > 0.0))
    return (int)hipErrorInvalidValue;
  const double kt = 0.0019872067 * t_target, ket = tdof * kt;
  return launch(nh_chain_kernel, dim3(1), 256, stream, state, work, npart, t_target, tdof, kt, ket, *params);
}

int ani_md_nh_scale(double* v, int nlocal, const double* state, void* stream) {
  if (nlocal <= 0) return 0;
  if (!v || !state) return (int)hipErrorInvalidValue;
  return launch(nh_scale_kernel, blocks(3 * nlocal), 256, stream, v, nlocal, state);
}

int ani_md_nh_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                                const double* x_built, double* d2max, const double* state, void* stream) {
  if (nlocal <= 0) return 0;
  if (!state) return (int)hipErrorInvalidValue;
  return launch(nh_initial_integrate_kernel, blocks(nlocal), 256, stream, x, v, f, dtfm, dt, nlocal, x_built, d2max, state);
}

int ani_md_nh_final_integrate(double* v, const double* f, const double* dtfm, const double* mass, int nlocal, double* work,
                              void* stream) {
  if (nlocal <= 0) return 0;
  if (!mass || !work) return (int)hipErrorInvalidValue;
  return launch(nh_final_integrate_kernel, blocks(nlocal), 256, stream, v, f, dtfm, mass, nlocal, work);
}

int ani_md_npt_init(double* npt_state, const double* lo3, const double* len3, int nlocal, void* stream) {
  if (!npt_state || !lo3 || !len3 || nlocal <= 0) return (int)hipErrorInvalidValue;
  for (int k = 0; k < 3; k++)
    if (!(len3[k] > 0.0) || !(len3[k] - len3[k] == 0.0) || !(lo3[k] - lo3[k] == 0.0)) return (int)hipErrorInvalidValue;
  return launch(npt_init_kernel, dim3(1), 1, stream, npt_state, lo3[0], lo3[1], lo3[2], len3[0], len3[1], len3[2], (double)nlocal);
}

int ani_md_npt_chain(int phase, double* nh_state, double* npt_state, const double* work, int npart, const double* ev, double t_target,
                     double p_target, double tdof, const ani_md_npt_params* params, void* stream) {
  if (!nh_state || !npt_state || !ev || !params || npart < 0 || (npart > 0 && !work) || (phase != 0 && phase != 1))
    return (int)hipErrorInvalidValue;
  const ani_md_npt_params& q = *params;
  if (q.mtchain < 1 || q.mtchain > ANI_MD_NH_MAXCHAIN || q.mpchain < 1 || q.mpchain > ANI_MD_NH_MAXCHAIN || q.nc_tchain < 1 ||
      q.nc_pchain < 1 || !(q.t_period > 0.0) || !(q.p_period > 0.0) || !(q.dt > 0.0) || !(t_target > 0.0) || !(tdof > 0.0) ||
      !(p_target - p_target == 0.0))
    return (int)hipErrorInvalidValue;
  const double kt = 0.0019872067 * t_target, ket = tdof * kt;
  return launch(npt_chain_kernel, dim3(1), 256, stream, phase, nh_state, npt_state, work, npart, ev, t_target, p_target, tdof, kt, ket, q);
}

int ani_md_npt_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                                 const double* x_built, double* d2max, const double* nh_state, const double* npt_state,
                                 double* shift, int nghost, void* stream) {
  if (nghost < 0) return (int)hipErrorInvalidValue;
  if (nlocal <= 0) return 0;
  if (!nh_state || !npt_state || (nghost > 0 && !shift)) return (int)hipErrorInvalidValue;
  return launch(npt_initial_integrate_kernel, blocks(nlocal + nghost), 256, stream, x, v, f, dtfm, dt, nlocal, x_built, d2max, nh_state,
                npt_state, shift, nghost);
}

int ani_md_npt_final_integrate(double* v, const double* f, const double* dtfm, const double* mass, int nlocal,
                               const double* npt_state, double* work, void* stream) {
  if (nlocal <= 0) return 0;
  if (!mass || !work || !npt_state) return (int)hipErrorInvalidValue;
  return launch(npt_final_integrate_kernel, blocks(nlocal), 256, stream, v, f, dtfm, mass, nlocal, npt_state, work);
}

int ani_md_npt_check(double* d2max, const double* ev, const double* npt_state, double* out, void* stream) {
  if (!npt_state) return (int)hipErrorInvalidValue;
  return launch(npt_check_kernel, dim3(1), 1, stream, d2max, ev, npt_state, out);
}

int ani_md_thermo_work_size(int nlocal) { return 6 * nblocks(nlocal); }

int ani_md_thermo(const double* v, const double* mass, int nlocal, const double* ev, int with_virial, double tdof, double volume,
                  const double* nh_state, double* work, double* out, void* stream) {
  if (!ev || !out || (nlocal > 0 && (!v || !mass || !work))) return (int)hipErrorInvalidValue;
  const int nblk = nlocal > 0 ? (nlocal + 255) / 256 : 0;
  if (nblk) enqueue(thermo_reduce_kernel, dim3(nblk), 256, stream, v, mass, nlocal, work);
  return launch(thermo_finish_kernel, dim3(1), 256, stream, work, nblk, ev, with_virial, tdof, volume, nh_state, out);
}

}  // extern "C"
