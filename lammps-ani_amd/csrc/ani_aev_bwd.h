// ani_aev_bwd.h — analytic backward pass of the AEV fast path: the force and per-atom virial scatters, backward_centre,
// aev_backward_fast (the design: head of ani_aev_device.h).  Kernel templates; ani_kernels_aev_fast.hip instantiates them.
#pragma once
#include <type_traits>

#include "ani_aev_stream.h"

namespace ani {

// one add to a neighbour's fp64 gradient accumulator in LDS (FastLds::gd)
__device__ __forceinline__ void gd_add(double* p, float v) { atomicAdd(p, (double)v); }

// coalesced force scatter of `cnt` neighbours whose gradients sit in LDS as g[3*q + k] with atom indices jx[q]:
// lane = (list slot, component), so the three adds of one atom (one float4 of fbuf) leave from adjacent lanes of ONE
// instruction.  Global float atomics execute at the memory side as 64-byte requests (MI355X_MICROARCH.md): three
// separate instructions per neighbour were three requests, this is one, and atoms adjacent both in memory and in the
// (spatially ordered) list share requests too.
template <typename T>
__device__ __forceinline__ void scatter_neighbours(const AevArgs& a, const T* g, const int* jx, int cnt, int lane) {
  for (int base = 0; base < cnt; base += 16) {
    const int q = base + (lane >> 2), k = lane & 3;
    if (q < cnt && k < 3) atomicAdd(&a.fbuf[4 * jx[q] + k], -(float)g[3 * q + k]);
  }
}

// Per-atom virial (ani_request_atom_virial): the same shape for the nine products of a scattered neighbour -- lane = (list slot,
// component), an atom's nine adds leave from nine adjacent lanes of ONE instruction, seven atoms per instruction.
// avir[9 j + 3 a + b] += d_a g_b with d = x_j - x_centre (float d[vs * q + a]) and g = dE_centre/dx_j: minus the site-energy
// virial (x_j - x_i) (x) F_j^(i) in Hartree (the conversion kernel applies sign, units and component order)
template <typename T, typename D>
__device__ __forceinline__ void scatter_atom_virial(float* __restrict__ avir, const T* g, const D* d, int vs, const int* jx, int cnt,
                                                    int lane) {
  const int qs = lane / 9, k = lane - 9 * qs, ca = k / 3, cb = k - 3 * ca;
  for (int base = 0; base < cnt; base += 7) {
    const int q = base + qs;
    if (qs < 7 && q < cnt) atomicAdd(&avir[9 * (long long)jx[q] + k], (float)d[vs * q + ca] * (float)g[3 * q + cb]);
  }
}

// AV: per-atom virial into avir[ntotal][9] (see scatter_atom_virial); vt: [3*64] LDS staging of the radial-only displacements
// TAB, sc: the centre's place in the backward stream table (sc.on), requested by the caller with the centre's lists
template <int NA, int NZ, int NCH, int GR, bool VIR, bool AV, bool TAB, typename PF>
__device__ __forceinline__ void backward_centre(const AevParams& p, const AevArgs& a, FastLds& L, int row, const hdr_t h,
                                                const Loaded<NCH, true, GR> pf, int lane, float (&wv)[9],
                                                const RepTab& rep, float* __restrict__ avir, float* vt, float& er, StreamCur sc,
                                                PF&& before_final_scatter BWD_STAMP_PARAMS) {
  constexpr int NR = 16;
  const int centre = h[0];
  const int nrad = hdr_nrad(h), nang = hdr_nang(h);
  // the rows of the neighbours that are centres themselves (symmetric radial collection, below): asked for here, in front of
  // the centre's set-up, instead of inside the radial stage -- where the lookup stood between the entry and the row it selects,
  // two dependent round trips in a row
  int rjp[NCH];
#pragma unroll
  for (int k = 0; k < NCH; k++) {
    rjp[k] = -1;
    if (a.row_of_atom && 64 * k + lane < nrad) rjp[k] = a.row_of_atom[cl_index(pf.jj[k])];
  }
#pragma unroll
  for (int c = 0; c < GR; c++)
    if (lane + 64 * c < (p.aev_stride >> 2)) reinterpret_cast<float4*>(L.row)[lane + 64 * c] = pf.grow[c];
  {
    // starts of the species groups in the angular list (the pair table is built from them): lane s takes its count out of the
    // header and a three-level DPP scan makes the prefix; lane S ends up with the total
    const int word = lane < 4 ? h[2] : h[3];
    const int ca = lane < 8 ? (word >> (8 * (lane & 3))) & 0xff : 0;
    int inc = ca;
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, true);   // row_shr:1
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, true);   // row_shr:2
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, true);   // row_shr:4
    if (lane <= p.S) L.astart[lane] = inc - ca;
  }
  wave_sync();   // the dE/dAEV row is read below

  // ---- radial stage, one lane per neighbour, straight from the prefetched registers.  A radial-only neighbour
  // (Rca < r <= Rcr) is finished here: its gradient goes to the centre's sums and, through a 64-slot staging buffer,
  // to the force scatter.  A neighbour inside Rca parks its displacement, atom index and radial gradient in LDS, where
  // the angular stage adds to it. ----
  float fx = 0.f, fy = 0.f, fz = 0.f;   // this lane's share of sum_j g_j (force on the centre)
  float ov[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // AV: the centre's own row, d (x) gs of the symmetric collection
  const float cR = -p.EtaR * kLog2e;
  const float rev = 0.5f * p.pi_over_Rcr * 0.3183098861837907f;
  const float revA = 0.5f * p.pi_over_Rca * 0.3183098861837907f;
  const float4* __restrict__ px = a.cl_xyz + (size_t)row * a.cl_stride;
  const int* __restrict__ pj = a.cl_j + (size_t)row * a.cl_stride;
  // chunks of the compact list in slot order: lanes with t < nang hold angular neighbours, the others radial-only ones
  for (int base = 0; base < nrad; base += 64) {
    const int c = base >> 6, t0 = base + lane;
    const bool live = t0 < nrad, ang = t0 < nang;
    const int w = ang ? t0 : t0 - nang;   // index in its stream
    float4 v = make_float4(0.f, 0.f, 0.f, 1.f);
    int j = 0;
    if (c < NCH) {
#pragma unroll
      for (int k = 0; k < NCH; k++)
        if (c == k) { v = pf.xx[k]; j = pf.jj[k]; }
    } else if (live) {  // lists longer than the chunks held in registers: loaded in place
      v = px[slot_index(t0, nang)];
      j = pj[slot_index(t0, nang)];
    }
    const int t = w;   // angular neighbours: index of the LDS accumulators
    float gx = 0.f, gy = 0.f, gz = 0.f;
    const int s = cl_species(j);   // the entry carries its species (cl_pack)
    j = cl_index(j);
    // A pair's two radial terms -- E_centre's and E_neighbour's dependence on their distance -- differ only in the dE/dAEV
    // row they are weighted with (same Gaussians, same cutoff factor).  When the neighbour is a centre of this launch too, the
    // centre reads the neighbour's row (its block for the centre's species) and takes BOTH terms' force on itself; the
    // neighbour does the same from its side, and neither scatters a radial gradient to the other: two thirds of the kernel's
    // global atomics were those (it waits for its atomics, not for its arithmetic).  Ghosts have no row here: their term is
    // scattered as before and comes back through the ghost exchange.  sym: this lane's neighbour is handled that way.
    float gsx = 0.f, gsy = 0.f, gsz = 0.f;   // sym: what the centre adds to its own force beyond (gx, gy, gz)
    int rj = -1;
    if (c < NCH) {
#pragma unroll
      for (int k = 0; k < NCH; k++)
        if (c == k) rj = rjp[k];
    } else if (a.row_of_atom && live) rj = a.row_of_atom[j];
    const bool sym = rj >= 0;
    if (live) {
      const float4* gg4 = reinterpret_cast<const float4*>(L.row + s * NR);
      const float4* qq4 = reinterpret_cast<const float4*>(a.gaev + (size_t)(sym ? rj : row) * p.aev_stride + hdr_species(h) * NR);
      const float r = v.w;
      const float fc = 0.5f * fcos_rev(r * rev) + 0.5f;
      const float dfc = -0.5f * p.pi_over_Rcr * fsin_rev(r * rev);
      float dEdr = 0.f, dEdn = 0.f;   // d/dr of the centre's energy, of the neighbour's
      // The sixteen Gaussians exp2(cR (r - ShfR_k)^2) from six exponentials: in each half of the shifts, around its midpoint
      // sc, d_k = dc - m Delta (m = k - 3.5) and exp2(cR d_k^2) = E H^(2m) C_|m| with E = exp2(cR dc^2), H = exp2(-cR dc Delta),
      // C_m = exp2(cR m^2 Delta^2) (wave-uniform).  A transcendental takes the issue time of ~5 FMAs (tools/issue_probe.hip).
      // E H^(2m) <= 1 / C_m; when E underflows, the half's largest term is below exp(-EtaR (|dc| - 3.5 Delta)^2) ~ 1e-12.
      {
        const float cd = cR * p.dShfR * p.dShfR;
        const float C0 = fexp2(0.25f * cd), C1 = fexp2(2.25f * cd), C2 = fexp2(6.25f * cd), C3 = fexp2(12.25f * cd);
        const float kf = -2.f * p.EtaR * fc;
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
          const float dc = r - (p.ShfR0 + (3.5f + 8.f * hf) * p.dShfR);
          const float x = cR * dc;
          const float E = fexp2(x * dc), H = fexp2(-x * p.dShfR), Hi = fexp2(x * p.dShfR);
          const float R = H * H, Ri = Hi * Hi;
          float e[8];
          float up = E * H, dn = E * Hi;
          e[4] = up * C0; up *= R; e[5] = up * C1; up *= R; e[6] = up * C2; up *= R; e[7] = up * C3;
          e[3] = dn * C0; dn *= Ri; e[2] = dn * C1; dn *= Ri; e[1] = dn * C2; dn *= Ri; e[0] = dn * C3;
          const float4 ga = gg4[2 * hf], gb = gg4[2 * hf + 1];
          const float gk[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
          float4 qa = make_float4(0.f, 0.f, 0.f, 0.f), qb = qa;
          if (sym) { qa = qq4[2 * hf]; qb = qq4[2 * hf + 1]; }
          const float qk[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
          float dr = dc + 3.5f * p.dShfR;   // r - ShfR[8 hf]
#pragma unroll
          for (int kk = 0; kk < 8; kk++) {
            const float tk = e[kk] * fmaf(kf, dr, dfc);
            dEdr = fmaf(gk[kk], tk, dEdr);
            dEdn = fmaf(qk[kk], tk, dEdn);
            dr -= p.dShfR;
          }
        }
      }
      const float inv_r = frcp(r);
      const float sc = 0.25f * dEdr * inv_r, scn = 0.25f * dEdn * inv_r;
      gx = sc * v.x; gy = sc * v.y; gz = sc * v.z;
      gsx = scn * v.x; gsy = scn * v.y; gsz = scn * v.z;
      if (rep.on && r < rep.cutoff) {
        // pairwise repulsion (ani_kernels_rep.hip has the formulas): half of e(r) per list entry.  The pair function in
        // fp32 like the rest of this precision mode, but its argument from the fp64 positions: the wall is steep
        const int ti = 8 * hdr_species(h) + s;
        const double* xj = rep.x64 + 3 * (long long)j;
        const double* xc = rep.x64 + 3 * (long long)centre;
        const double ddx = xj[0] - xc[0], ddy = xj[1] - xc[1], ddz = xj[2] - xc[2];
        const double r64 = sqrt(ddx * ddx + ddy * ddy + ddz * ddz);
        const float rr = (float)r64;
        const float x = rr * frcp(rep.cutoff), den = 1.f - x * x;
        if (den > 1e-10f) {
          const float fcr = fexp2((1.f - frcp(den)) * kLog2e);
          const float dfcr = fcr * (-(2.f * x * frcp(rep.cutoff)) * frcp(den * den));
          const float db = rr * 1.8897261258369282f, al = rep.sa[ti], kk = rep.k[ti];
          const float pk1 = fexp2((kk - 1.f) * flog2(db));
          const float g = rep.y[ti] * frcp(db) * fexp2(-al * pk1 * db * kLog2e);
          const float dg = 1.8897261258369282f * g * (-frcp(db) - al * kk * pk1);
          er += 0.5f * g * fcr;
          const float sr = 0.5f * (dg * fcr + g * dfcr);
          const double inv = 1.0 / r64;
          const float rx = sr * (float)(ddx * inv), ry = sr * (float)(ddy * inv), rz = sr * (float)(ddz * inv);
          gx += rx; gy += ry; gz += rz;
          if (sym) { gsx += rx; gsy += ry; gsz += rz; }   // the neighbour's entry for this pair holds the same half of the pair term
        }
      }
    }
    if constexpr (AV) {
      // the neighbour's term lands on the centre itself: (x_i - x_j) (x) gs in the centre's own row, from registers (gs = 0 unless
      // sym); the neighbour's wave adds the mirror image to its row
      ov[0] += v.x * gsx; ov[1] += v.x * gsy; ov[2] += v.x * gsz;
      ov[3] += v.y * gsx; ov[4] += v.y * gsy; ov[5] += v.y * gsz;
      ov[6] += v.z * gsx; ov[7] += v.z * gsy; ov[8] += v.z * gsz;
    }
    if (live && ang) {
      L.ad[t] = v;
      L.afc[t] = 0.5f * fcos_rev(v.w * revA) + 0.5f;
      L.aj[t] = j;
      if (sym) {   // radial terms settled here on the centre's side; the accumulator starts empty for the angular stage
        fx += gx + gsx; fy += gy + gsy; fz += gz + gsz;
        if constexpr (VIR) {
          wv[0] += gx * v.x; wv[1] += gx * v.y; wv[2] += gx * v.z;
          wv[3] += gy * v.x; wv[4] += gy * v.y; wv[5] += gy * v.z;
          wv[6] += gz * v.x; wv[7] += gz * v.y; wv[8] += gz * v.z;
        }
        gx = gy = gz = 0.f;
      }
      L.gd[3 * t] = gx; L.gd[3 * t + 1] = gy; L.gd[3 * t + 2] = gz;
    }
    // radial-only neighbours: finished here (scattered at once; ONE merged scatter per centre -- angular + radial-only +
    // centre, 21 atoms per atomic instruction instead of 16 -- was measured: 5 % slower, the atomics then leave in one
    // burst at the end of the centre instead of two spread over it)
    const int lo = min(max(nang - base, 0), 64), hi = min(nrad - base, 64);   // radial-only lanes of this chunk: [lo, hi)
    if (hi > lo) {   // wave-uniform
      const bool out = live && !ang && !sym;            // a radial-only neighbour whose gradient has to travel
      const unsigned long long mout = __ballot(out);
      if (live && !ang) {
        fx += gx + gsx; fy += gy + gsy; fz += gz + gsz;   // (gs = 0 unless sym)
        if constexpr (VIR) {
          wv[0] += gx * v.x; wv[1] += gx * v.y; wv[2] += gx * v.z;
          wv[3] += gy * v.x; wv[4] += gy * v.y; wv[5] += gy * v.z;
          wv[6] += gz * v.x; wv[7] += gz * v.y; wv[8] += gz * v.z;
        }
        if (out) {
          const int q = lanes_below(mout);
          L.gt[3 * q] = gx; L.gt[3 * q + 1] = gy; L.gt[3 * q + 2] = gz;
          L.jt[q] = j;
          if constexpr (AV) { vt[3 * q] = v.x; vt[3 * q + 1] = v.y; vt[3 * q + 2] = v.z; }
        }
      }
      wave_sync();
      scatter_neighbours(a, L.gt, L.jt, __popcll(mout), lane);
      if constexpr (AV) scatter_atom_virial(avir, L.gt, vt, 3, L.jt, __popcll(mout), lane);
      wave_sync();   // the staging buffer is reused by the next chunk
    }
  }
  BWD_STAMP(2);   // radial stage incl. the radial-only scatter
  // ---- angular, dense pair stream (round 3).  The pairs of all non-empty species-pair buckets form ONE stream, bucket after
  // bucket, that a step takes 64 lanes of whatever buckets they belong to: a water centre's 153 pairs are 3 steps (the row
  // layout it replaced, one 16-lane row per row neighbour, needed 4: 60 % of its lanes held a pair; summing a column's four
  // rows in registers before one conflict-free add was slower still, 0.434 against 0.407 ms, and so was parking the row sums
  // in LDS for one add per block of rows: profiles/r02_ablation_notes.md).  The two half-waves walk the stream's column slots
  // together, on two adjacent row neighbours (build_pair_table).  The pairs of a half-wave that share their ROW neighbour are
  // consecutive lanes (a run): its gradient is summed over the run by a segmented scan inside each 16-lane DPP row -- level d
  // adds the value d lanes down if that lane belongs to the same run -- and the last lane of the run in its DPP row adds the
  // partial sum to the neighbour's LDS accumulator.  The COLUMN neighbour's gradient: one LDS add per lane.
  int nbk = 0, total_pairs;
  bool tabbed = false;   // wave-uniform: this centre's slots come from the stream table
  if constexpr (TAB) tabbed = sc.on;
  if (tabbed) {
    total_pairs = sc.total;
  } else {
    total_pairs = build_pair_table<NA, NZ>(p, lane, L, nbk);
    wave_sync();
  }
  BWD_STAMP(3);   // pair table
  const float cA = -p.EtaA * kLog2e;
  for (int base = 0; base < total_pairs; base += 32) {
    int ia, ib, outoff, pos;
    bool valid;
    if (tabbed) {   // the word requested two steps ago; the one of the step after the next leaves now
      const unsigned w = sc.w0;
      sc.w0 = sc.w1;
      if (base + 64 < total_pairs) sc.w1 = sc.wp[base + 64 + (lane & 31)];
      const int hh = lane >> 5;
      valid = (w >> (30 + hh)) & 1;
      const int up = valid ? hh : 0;   // an idle upper half stays on the even row's pair: a harmless geometry
      ia = (int)(w & 0xff) + up;
      ib = (w >> 8) & 0xff;
      pos = valid ? (int)((w >> 16) & 0xff) - (int)((w >> 29) & (unsigned)up) : 0;
      outoff = p.radial_len + (int)((w >> 24) & 0x1f) * (NA * NZ);
    } else {
      stream_pair_half(L, nbk, base + (lane & 31), lane >> 5, ia, ib, outoff, pos, valid);
    }
    const float4 A = L.ad[ia], B = L.ad[ib];
    const float inv_ra = frcp(A.w), inv_rb = frcp(B.w);
    const float inv_rr = inv_ra * inv_rb;
    const float cosv = (A.x * B.x + A.y * B.y + A.z * B.z) * inv_rr;
    const float c = 0.95f * cosv;
    const float s2 = fmaxf(1.f - c * c, 1e-12f);
    const float inv_s = frsq(s2);
    const float sn = s2 * inv_s;
    const float fa = L.afc[ia], fb = L.afc[ib];
    const float dfa = -0.5f * p.pi_over_Rca * fsin_rev(A.w * revA);
    const float dfb = -0.5f * p.pi_over_Rca * fsin_rev(B.w * revA);
    const float rho = 0.5f * (A.w + B.w);
    float f1[NZ], df1[NZ];
#pragma unroll
    for (int z = 0; z < NZ; z++) {
      const float bz = fmaxf(0.5f * (1.f + c * p.cosZ[z] + sn * p.sinZ[z]), 0.f);
      const float pm1 = fexp2((p.Zeta - 1.f) * flog2(bz));
      f1[z] = pm1 * bz;
      df1[z] = p.Zeta * pm1 * 0.5f * (sn * p.cosZ[z] - c * p.sinZ[z]) * inv_s;
    }
    const float4* gg4 = reinterpret_cast<const float4*>(L.row + outoff);  // outoff is a multiple of NA*NZ
    float Aq = 0.f, Bq = 0.f, Cq = 0.f;
    float drA = rho - p.ShfA0;
#pragma unroll
    for (int sa = 0; sa < NA; sa++) {
      const float dr = drA;
      drA -= p.dShfA;   // equidistant shifts
      const float f2 = fexp2(cA * dr * dr);
      const float df2 = -2.f * p.EtaA * dr * f2;
      float g1 = 0.f, gd1 = 0.f;
#pragma unroll
      for (int z4 = 0; z4 < NZ / 4; z4++) {
        const float4 gv = gg4[sa * (NZ / 4) + z4];
        g1 = fmaf(gv.x, f1[4 * z4], g1); gd1 = fmaf(gv.x, df1[4 * z4], gd1);
        g1 = fmaf(gv.y, f1[4 * z4 + 1], g1); gd1 = fmaf(gv.y, df1[4 * z4 + 1], gd1);
        g1 = fmaf(gv.z, f1[4 * z4 + 2], g1); gd1 = fmaf(gv.z, df1[4 * z4 + 2], gd1);
        g1 = fmaf(gv.w, f1[4 * z4 + 3], g1); gd1 = fmaf(gv.w, df1[4 * z4 + 3], gd1);
      }
      Aq = fmaf(f2, gd1, Aq);
      Cq = fmaf(f2, g1, Cq);
      Bq = fmaf(df2, g1, Bq);
    }
    // gradient of this pair w.r.t. the two neighbour displacements; zero for masked lanes
    const float P = valid ? fa * fb : 0.f;
    Aq *= 2.f * P * 0.95f;
    Bq *= P;       // 2 * P * 0.5
    Cq *= valid ? 2.f : 0.f;
    const float cc = Aq * inv_rr;
    const float ta = (Bq + Cq * dfa * fb) * inv_ra - Aq * cosv * inv_ra * inv_ra;
    const float tb = (Bq + Cq * fa * dfb) * inv_rb - Aq * cosv * inv_rb * inv_rb;
    const float va[3] = {cc * B.x + ta * A.x, cc * B.y + ta * A.y, cc * B.z + ta * A.z};  // d/d(neighbour ia)
    const float vb[3] = {cc * A.x + tb * B.x, cc * A.y + tb * B.y, cc * A.z + tb * B.z};  // d/d(neighbour ib)
    // column neighbour: lanes l and l + 32 hold the same one.  One fp64 LDS add per lane and component (the two half-waves'
    // lanes l, l + 32 share the address: a two-way conflict costs less than the half-wave swap-add that used to halve the
    // number of slow fp32 adds)
    if (valid) { gd_add(&L.gd[3 * ib], vb[0]); gd_add(&L.gd[3 * ib + 1], vb[1]); gd_add(&L.gd[3 * ib + 2], vb[2]); }
    // row neighbour: segmented inclusive scan over the run, inside the lane's 16-lane DPP row
    float rs[3] = {va[0], va[1], va[2]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
      // the DPP move is executed by every lane (it is a cross-lane read: inside a conditional it would see the lanes the
      // condition switched off as invalid sources); the condition only selects what is added
      float t;
      t = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(rs[k]), 0x111, 0xf, 0xf, true)); rs[k] += pos >= 1 ? t : 0.f;   // row_shr:1
      t = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(rs[k]), 0x112, 0xf, 0xf, true)); rs[k] += pos >= 2 ? t : 0.f;   // row_shr:2
      t = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(rs[k]), 0x114, 0xf, 0xf, true)); rs[k] += pos >= 4 ? t : 0.f;   // row_shr:4
      t = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(rs[k]), 0x118, 0xf, 0xf, true)); rs[k] += pos >= 8 ? t : 0.f;   // row_shr:8
    }
    // the run ends here (for this DPP row) if the next lane starts a run or lies in the next DPP row
    const int pos_next = __builtin_amdgcn_update_dpp(0, pos, 0x101, 0xf, 0xf, true);   // row_shl:1: lane 15 of a row reads 0
    if (valid && pos_next == 0) { gd_add(&L.gd[3 * ia], rs[0]); gd_add(&L.gd[3 * ia + 1], rs[1]); gd_add(&L.gd[3 * ia + 2], rs[2]); }
  }
  wave_sync();   // gd is complete
  BWD_STAMP(4);   // angular stage
  // ---- the angular neighbours: F_j -= gd_j ; F_i += sum_j gd_j ; virial -= gd (x) d ----
  for (int q = lane; q < nang; q += 64) {
    const float gx = (float)L.gd[3 * q], gy = (float)L.gd[3 * q + 1], gz = (float)L.gd[3 * q + 2];
    fx += gx; fy += gy; fz += gz;
    if constexpr (VIR) {
      // virial: per-lane partial sums kept across all the centres of this wave; the nine totals are reduced over the
      // lanes and added to the global accumulator ONCE per wave at the end of the kernel (nine double atomics per centre
      // on nine addresses serialise at the memory side: 10 ms per step at 100 000 centres)
      const float4 d = L.ad[q];
      wv[0] += gx * d.x; wv[1] += gx * d.y; wv[2] += gx * d.z;
      wv[3] += gy * d.x; wv[4] += gy * d.y; wv[5] += gy * d.z;
      wv[6] += gz * d.x; wv[7] += gz * d.y; wv[8] += gz * d.z;
    }
  }
  before_final_scatter();   // the caller's loads for the wave's next centre: in front of the atomics in the in-order memory queue
  scatter_neighbours(a, L.gd, L.aj, nang, lane);
  if constexpr (AV) {
    scatter_atom_virial(avir, L.gd, reinterpret_cast<const float*>(L.ad), 4, L.aj, nang, lane);
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const float t = xor_sum<32>(xor_sum<16>(xor_sum<8>(xor_sum<4>(xor_sum<2>(xor_sum<1>(ov[k]))))));
      if (lane == k) mine = t;
    }
    if (lane < 9) atomicAdd(&avir[9 * (long long)centre + lane], mine);
  }
  fx = xor_sum<32>(xor_sum<16>(xor_sum<8>(xor_sum<4>(xor_sum<2>(xor_sum<1>(fx))))));
  fy = xor_sum<32>(xor_sum<16>(xor_sum<8>(xor_sum<4>(xor_sum<2>(xor_sum<1>(fy))))));
  fz = xor_sum<32>(xor_sum<16>(xor_sum<8>(xor_sum<4>(xor_sum<2>(xor_sum<1>(fz))))));
  if (lane < 3) atomicAdd(&a.fbuf[4 * centre + lane], lane == 0 ? fx : (lane == 1 ? fy : fz));
  wave_sync();  // the LDS slice is reused by this wave's next centre
  BWD_STAMP(5);   // final scatter
}


// AVP: empty, float* for the armed instantiation (per-atom virial accumulator), StreamTab for the ones with stream tables, or both
// (StreamTab first) -- a parameter pack, so that the unarmed kernels without tables keep their argument list, and with it their
// instruction stream, exactly as it was
__device__ __forceinline__ void take_extra(StreamTab&, float*&) {}
template <typename... R>
__device__ __forceinline__ void take_extra(StreamTab& t, float*& av, float* x, R... r) { av = x; take_extra(t, av, r...); }
template <typename... R>
__device__ __forceinline__ void take_extra(StreamTab& t, float*& av, StreamTab x, R... r) { t = x; take_extra(t, av, r...); }
template <typename T, typename... P> constexpr bool pack_has = (std::is_same<T, P>::value || ...);

template <int NA, int NZ, int NCH, int GR, bool VIR, typename... AVP>
__global__ __launch_bounds__(64 * kWavesB, kBwdMinWaves) void aev_backward_fast(AevParams p, AevArgs a, int cap, int rowf, RepTab rep,
                                                                                AVP... avp) {
  constexpr bool AV = pack_has<float*, AVP...>, TAB = pack_has<StreamTab, AVP...>;
  float* avir = nullptr;
  StreamTab tab{};
  take_extra(tab, avir, avp...);
  extern __shared__ float4 smem4[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // the centre's place in the backward stream table, from the count bytes of its header (scalar)
  auto stream_of = [&](const hdr_t& hx) -> StreamCur {
    if constexpr (TAB) return stream_begin<32>(tab.desc_b, tab.words_b, stream_tuple(p, tab, hx[2] & 0xff, (hx[2] >> 8) & 0xff), lane);
    else return StreamCur{};
  };
  float* wbase = reinterpret_cast<float*>(smem4) + wave * bwd_wave_floats(cap, rowf, p.S, AV);
  FastLds L = carve<NA, NZ>(wbase, cap, true, rowf);
  float* vt = AV ? wbase + fast_wave_floats_row(cap, true, rowf, p.S) : nullptr;
  float wv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // this lane's share of the wave's virial
  float er = 0.f;                                                // ... and of its repulsion energy
#ifdef ABLB_STAMPS
  unsigned long long stamp_prev, stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory");
  const int nw = gridDim.x * kWavesB;
  for (int k = blockIdx.x * kWavesB + wave; k < a.kcount; k += nw) {
    const int row = ticket_row(a, k);
    const hdr_t hc = load_header(a, row);
    BWD_STAMP(0);   // header (waits for whatever this wave still has in flight: the last centre's atomics)
    if (hc[0] < 0) continue;
    Loaded<NCH, true, GR> cur;
    load_lists(p, a, row, hdr_nrad(hc), hdr_nang(hc), lane, cur);
#ifdef ABLB_STAMPS_VM
    BWD_STAMP_VM(1);   // list + dE/dAEV row
#else
    BWD_STAMP(1);
#endif
    backward_centre<NA, NZ, NCH, GR, VIR, AV, TAB>(p, a, L, row, hc, cur, lane, wv, rep, avir, vt, er, stream_of(hc), [] {}, stamp_prev,
                                                   stamp_acc);
    stamp_acc[6] += 1;
  }
  if (wave == 0 && lane == 0) {
    for (int q = 0; q < 6; q++) atomicAdd(&g_bwd_stamps[q], stamp_acc[q]);
    atomicAdd(&g_bwd_stamps[8], stamp_acc[6]);
  }
#else
  // Persistent loop of the backward pass (rows by ticket, a group's rows interleaved with the other groups': ANI_PERSISTENT_LOOP).
  // A centre ends with its force atomics, and the memory queue is in order: loads issued behind them return behind them, so a
  // wave that asks for its next centre's lists AFTER the scatter waits a whole atomic round trip per centre (without the global
  // atomics the kernel takes 0.205 instead of 0.254 ms).  So the next centre's header (a scalar load: its own counter) and lists
  // are requested in front of the final scatter, when only the registers of the centre's tail are live.
  ANI_TICKETS_BEGIN(kWavesB)
  const int kstop = tk_ctr ? tk_base + tk_share : kend;
  auto rank_of = [&](int kx) -> int { return tk_ctr ? (kx - tk_base) * tk_ngrp + tk_grp : kx; };
  bool have = false;   // hc / cur already hold the centre of ticket k (requested in front of the previous centre's final scatter)
  hdr_t hc;
  Loaded<NCH, true, GR> cur;
  StreamCur sc;   // travels with hc / cur
  while (k < kstop) {
    ANI_TICKET_DRAW(tk_tn)
    const int kk = rank_of(k);
    const int row = ticket_row(a, kk);
    const bool in_range = kk < a.kcount;
    if (!have) {
      hc = load_header_scalar(a, row);
      if (hc[0] >= 0 && in_range) {
        load_lists(p, a, row, hdr_nrad(hc), hdr_nang(hc), lane, cur);
        sc = stream_of(hc);
      }
    }
    have = false;
    ANI_TICKET_TAKE(tk_k2)
    if (hc[0] >= 0 && in_range) {
      // header and lists go in by value: the hook overwrites hc / cur with the next centre's while this one finishes
      backward_centre<NA, NZ, NCH, GR, VIR, AV, TAB>(p, a, L, row, hc, cur, lane, wv, rep, avir, vt, er, sc, [&]() {
        const int kk1 = rank_of(k1);
        if (k1 < kstop && kk1 < a.kcount) {   // wave-uniform
          const int row1 = ticket_row(a, kk1);
          hc = load_header_scalar(a, row1);
          if (hc[0] >= 0) {
            load_lists(p, a, row1, hdr_nrad(hc), hdr_nang(hc), lane, cur);
            sc = stream_of(hc);   // first slot words of the next centre: in front of this centre's atomics, like its lists
          }
          have = true;
        }
      });
    }
    ANI_TICKET_NEXT(tk_tn, tk_k2)
  }
  ANI_TICKETS_END(kWavesB)
#endif
  if (rep.on) {
    double se = (double)er;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) se += __shfl_xor(se, off);
    if (lane == 0) atomicAdd(&rep.erep[(blockIdx.x * kWavesB + wave) & (kVirialSlots - 1)], se);
  }
  if constexpr (VIR) {
    if (a.virial) {
#pragma unroll
      for (int k = 0; k < 9; k++) {
        double sv = (double)wv[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sv += __shfl_xor(sv, off);
        if (lane == 0) atomicAdd(&a.virial[9 * ((blockIdx.x * kWavesB + wave) & (kVirialSlots - 1)) + k], -sv);
      }
    }
  }
}

}  // namespace ani
