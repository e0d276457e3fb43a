// ani_kernels_aev_generic.hip — AEV forward and backward for any model shape: the first-generation kernels, taken where the
// fast path does not apply (the design: head of ani_aev_device.h).
#include "ani_aev_launch.h"

namespace ani {

// =====================================================================================================
// generic path (any model shape): LDS float atomics, precise libm transcendentals
// =====================================================================================================
struct WaveLds {
  float dx[kMaxRad], dy[kMaxRad], dz[kMaxRad], r[kMaxRad], fc[kMaxRad];
  int sp[kMaxRad], j[kMaxRad];
  int ang[kMaxAng];
  float fca[kMaxAng];
  float row[kAevMax];
  float gd[3 * kMaxRad];
};

__device__ __forceinline__ void compact_neighbours(const AevParams& p, const AevArgs& a, int ii, int lane, WaveLds& L,
                                                   int& nrad, int& nang, bool& over) {
  const int i = a.ilist[ii];
  const float4 xi = a.xyzs[i];
  const int beg = a.nbr_off[ii];
  const int n = a.numneigh[ii];
  nrad = 0;
  nang = 0;
  over = false;
  for (int base = 0; base < n; base += 64) {
    const int q = base + lane;
    const bool valid = q < n;
    const int j = valid ? a.jlist[beg + q] : i;
    const float4 xj = a.xyzs[j];
    const float dx = xj.x - xi.x, dy = xj.y - xi.y, dz = xj.z - xi.z;
    const float r = sqrtf(dx * dx + dy * dy + dz * dz);
    const bool in_r = valid && (p.compat || r <= p.Rcr);
    const bool in_a = valid && r <= p.Rca;
    const unsigned long long mr = __ballot(in_r);
    const unsigned long long ma = __ballot(in_a);
    const int pos = nrad + lanes_below(mr);
    if (in_r && pos < kMaxRad) {
      L.dx[pos] = dx; L.dy[pos] = dy; L.dz[pos] = dz; L.r[pos] = r;
      L.fc[pos] = 0.5f * cosf(r * p.pi_over_Rcr) + 0.5f;
      L.sp[pos] = __float_as_int(xj.w);
      L.j[pos] = j;
    }
    const int posa = nang + lanes_below(ma);
    if (in_a && posa < kMaxAng && pos < kMaxRad) {
      L.ang[posa] = pos;
      L.fca[posa] = 0.5f * cosf(r * p.pi_over_Rca) + 0.5f;
    }
    nrad += __popcll(mr);
    nang += __popcll(ma);
  }
  if (nrad > kMaxRad) { nrad = kMaxRad; over = true; }
  if (nang > kMaxAng) { nang = kMaxAng; over = true; }
}

__global__ __launch_bounds__(64 * kWaves) void aev_forward_generic(AevParams p, AevArgs a) {
  __shared__ WaveLds lds[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWaves + wave;
  if (row >= a.nrows) return;
  const int ii = a.centre_of_row[row];
  if (ii < 0) return;
  WaveLds& L = lds[wave];

  for (int e = lane; e < p.aev_stride; e += 64) L.row[e] = 0.f;
  int nrad, nang;
  bool over;
  compact_neighbours(p, a, ii, lane, L, nrad, nang, over);
  if (over && lane == 0) atomicOr(a.err_flag, 1);
  wave_sync();

  const int nR = p.nR;
  for (int t = lane; t < nrad * nR; t += 64) {
    const int q = t / nR, k = t - q * nR;
    const float dr = L.r[q] - p.ShfR[k];
    const float v = 0.25f * expf(-p.EtaR * dr * dr) * L.fc[q];
    atomicAdd(&L.row[L.sp[q] * nR + k], v);
  }
  const int npair = nang * (nang - 1) / 2;
  for (int t = lane; t < npair; t += 64) {
    int ia, ib;
    decode_pair(t, nang, ia, ib);
    const int qa = L.ang[ia], qb = L.ang[ib];
    const float ra = L.r[qa], rb = L.r[qb];
    const float dot = L.dx[qa] * L.dx[qb] + L.dy[qa] * L.dy[qb] + L.dz[qa] * L.dz[qb];
    const float c = 0.95f * dot / fmaxf(ra * rb, 1e-10f);
    const float s = sqrtf(fmaxf(1.f - c * c, 0.f));
    const float w = 2.f * L.fca[ia] * L.fca[ib];
    const float rho = 0.5f * (ra + rb);
    float* out = &L.row[p.radial_len + triu_index(L.sp[qa], L.sp[qb], p.S) * p.nAZ];
    float f1[kMaxShfZ];
    for (int z = 0; z < p.nZ; z++) {
      const float base = 0.5f * (1.f + c * p.cosZ[z] + s * p.sinZ[z]);
      f1[z] = w * powf(fmaxf(base, 0.f), p.Zeta);
    }
    for (int sa = 0; sa < p.nA; sa++) {
      const float dr = rho - p.ShfA[sa];
      const float f2 = expf(-p.EtaA * dr * dr);
      for (int z = 0; z < p.nZ; z++) atomicAdd(&out[sa * p.nZ + z], f1[z] * f2);
    }
  }
  wave_sync();
  float* dst = a.aev + (long long)row * p.aev_stride;
  for (int e = lane; e < p.aev_stride; e += 64) dst[e] = L.row[e];
}

// AVP: empty, or float* for the armed instantiation: per-atom virial into avir[ntotal][9] (scatter_atom_virial's layout and sign)
template <typename... AVP>
__global__ __launch_bounds__(64 * kWaves) void aev_backward_generic(AevParams p, AevArgs a, AVP... avp) {
  constexpr bool AV = sizeof...(AVP) > 0;
  float* avir = nullptr;
  if constexpr (AV) avir = (avp, ...);
  __shared__ WaveLds lds[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWaves + wave;
  if (row >= a.nrows) return;
  const int ii = a.centre_of_row[row];
  if (ii < 0) return;
  WaveLds& L = lds[wave];

  const float* g = a.gaev + (long long)row * p.aev_stride;
  for (int e = lane; e < p.aev_stride; e += 64) L.row[e] = g[e];
  int nrad, nang;
  bool over;
  compact_neighbours(p, a, ii, lane, L, nrad, nang, over);
  if (over && lane == 0) atomicOr(a.err_flag, 1);
  wave_sync();

  const int nR = p.nR;
  for (int q = lane; q < nrad; q += 64) {
    const float r = L.r[q], fc = L.fc[q];
    const float dfc = -0.5f * p.pi_over_Rcr * sinf(r * p.pi_over_Rcr);
    const float* gg = &L.row[L.sp[q] * nR];
    float dEdr = 0.f;
    for (int k = 0; k < nR; k++) {
      const float dr = r - p.ShfR[k];
      const float e = 0.25f * expf(-p.EtaR * dr * dr);
      dEdr += gg[k] * e * (dfc - 2.f * p.EtaR * dr * fc);
    }
    const float s = dEdr / r;
    L.gd[3 * q + 0] = s * L.dx[q];
    L.gd[3 * q + 1] = s * L.dy[q];
    L.gd[3 * q + 2] = s * L.dz[q];
  }
  wave_sync();

  const int npair = nang * (nang - 1) / 2;
  for (int t = lane; t < npair; t += 64) {
    int ia, ib;
    decode_pair(t, nang, ia, ib);
    const int qa = L.ang[ia], qb = L.ang[ib];
    const float ra = L.r[qa], rb = L.r[qb];
    const float ax = L.dx[qa], ay = L.dy[qa], az = L.dz[qa];
    const float bx = L.dx[qb], by = L.dy[qb], bz = L.dz[qb];
    const float rr = ra * rb;
    const float cosv = (ax * bx + ay * by + az * bz) / rr;
    const float c = 0.95f * cosv;
    const float s = sqrtf(fmaxf(1.f - c * c, 1e-12f));
    const float fa = L.fca[ia], fb = L.fca[ib];
    const float dfa = -0.5f * p.pi_over_Rca * sinf(ra * p.pi_over_Rca);
    const float dfb = -0.5f * p.pi_over_Rca * sinf(rb * p.pi_over_Rca);
    const float P = fa * fb, rho = 0.5f * (ra + rb);
    const float* gg = &L.row[p.radial_len + triu_index(L.sp[qa], L.sp[qb], p.S) * p.nAZ];
    float f1[kMaxShfZ], df1[kMaxShfZ];
    for (int z = 0; z < p.nZ; z++) {
      const float base = fmaxf(0.5f * (1.f + c * p.cosZ[z] + s * p.sinZ[z]), 0.f);
      const float pm1 = powf(base, p.Zeta - 1.f);
      f1[z] = pm1 * base;
      df1[z] = p.Zeta * pm1 * 0.5f * (s * p.cosZ[z] - c * p.sinZ[z]) / s;
    }
    float A = 0.f, B = 0.f, C = 0.f;
    for (int sa = 0; sa < p.nA; sa++) {
      const float dr = rho - p.ShfA[sa];
      const float f2 = expf(-p.EtaA * dr * dr);
      const float df2 = -2.f * p.EtaA * dr * f2;
      for (int z = 0; z < p.nZ; z++) {
        const float gv = gg[sa * p.nZ + z];
        A = fmaf(gv * f2, df1[z], A);
        B = fmaf(gv * df2, f1[z], B);
        C = fmaf(gv * f2, f1[z], C);
      }
    }
    A *= 2.f * P * 0.95f;
    B *= 2.f * P * 0.5f;
    C *= 2.f;
    const float ca = A / rr, ia2 = A * cosv / (ra * ra), ib2 = A * cosv / (rb * rb);
    const float ta = (B + C * dfa * fb) / ra, tb = (B + C * fa * dfb) / rb;
    atomicAdd(&L.gd[3 * qa + 0], ca * bx + (ta - ia2) * ax);
    atomicAdd(&L.gd[3 * qa + 1], ca * by + (ta - ia2) * ay);
    atomicAdd(&L.gd[3 * qa + 2], ca * bz + (ta - ia2) * az);
    atomicAdd(&L.gd[3 * qb + 0], ca * ax + (tb - ib2) * bx);
    atomicAdd(&L.gd[3 * qb + 1], ca * ay + (tb - ib2) * by);
    atomicAdd(&L.gd[3 * qb + 2], ca * az + (tb - ib2) * bz);
  }
  wave_sync();

  float fx = 0.f, fy = 0.f, fz = 0.f;
  float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = lane; q < nrad; q += 64) {
    const float gx = L.gd[3 * q], gy = L.gd[3 * q + 1], gz = L.gd[3 * q + 2];
    const int j = L.j[q];
    atomicAdd(&a.fbuf[4 * j + 0], -gx);
    atomicAdd(&a.fbuf[4 * j + 1], -gy);
    atomicAdd(&a.fbuf[4 * j + 2], -gz);
    fx += gx; fy += gy; fz += gz;
    if (a.virial) {
      const float dx = L.dx[q], dy = L.dy[q], dz = L.dz[q];
      v[0] += gx * dx; v[1] += gx * dy; v[2] += gx * dz;
      v[3] += gy * dx; v[4] += gy * dy; v[5] += gy * dz;
      v[6] += gz * dx; v[7] += gz * dy; v[8] += gz * dz;
    }
  }
  if constexpr (AV) {   // every term is scattered here: (slot, component) lanes, nine adjacent lanes per atom
    const int qs = lane / 9, k = lane - 9 * qs, ca = k / 3, cb = k - 3 * ca;
    const float* dv = ca == 0 ? L.dx : (ca == 1 ? L.dy : L.dz);
    for (int base = 0; base < nrad; base += 7) {
      const int q = base + qs;
      if (qs < 7 && q < nrad) atomicAdd(&avir[9 * (long long)L.j[q] + k], dv[q] * L.gd[3 * q + cb]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    fx += __shfl_xor(fx, off);
    fy += __shfl_xor(fy, off);
    fz += __shfl_xor(fz, off);
  }
  const int i = a.ilist[ii];
  if (lane == 0) {
    atomicAdd(&a.fbuf[4 * i + 0], fx);
    atomicAdd(&a.fbuf[4 * i + 1], fy);
    atomicAdd(&a.fbuf[4 * i + 2], fz);
  }
  if (a.virial) {
#pragma unroll
    for (int k = 0; k < 9; k++) {
      float sv = v[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sv += __shfl_xor(sv, off);
      if (lane == 0) atomicAdd(&a.virial[k], -(double)sv);
    }
  }
}

void launch_aev_forward_generic(const AevParams& p, const AevArgs& a, hipStream_t st) {
  const dim3 grid((a.nrows + kWaves - 1) / kWaves), block(64 * kWaves);
  hipLaunchKernelGGL(aev_forward_generic, grid, block, 0, st, p, a);
}

void launch_aev_backward_generic(const AevParams& p, const AevArgs& a, hipStream_t st, float* avir) {
  const dim3 grid((a.nrows + kWaves - 1) / kWaves), block(64 * kWaves);
  if (avir) hipLaunchKernelGGL(aev_backward_generic<float*>, grid, block, 0, st, p, a, avir);
  else hipLaunchKernelGGL(aev_backward_generic<>, grid, block, 0, st, p, a);
}

}  // namespace ani
