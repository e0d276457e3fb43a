// ani_hip_model.cpp — the model on the device: weight upload, fp64 mirrors, 16-bit planes, specialize().  Internal: see ani_handle.h.
#include "ani_handle.h"

namespace ani_host __attribute__((visibility("hidden"))) {
int upload(ani_handle* h, float** dst, const std::vector<float>& src) {
  HIP_TRY(h, hipMalloc((void**)dst, std::max<size_t>(src.size(), 1) * sizeof(float)));
  HIP_TRY(h, hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
  return ANI_OK;
}

// precision 'double': the model file stores fp32 weights (exactly representable), so the fp64 copies are made on the
// device from the fp32 uploads
int mirror64(ani_handle* h, double** dst, const float* src, size_t n) {
  if (h->use_single) return ANI_OK;
  if (*dst) (void)hipFree(*dst);
  HIP_TRY(h, hipMalloc((void**)dst, std::max<size_t>(n, 1) * sizeof(double)));
  launch_cvt_f32_f64(src, *dst, n, h->stream);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return ANI_OK;
}

// device copies of `batch` matrices [N][ld] (first K columns) as blocked 16-bit planes, one per split arithmetic
int make_split(ani_handle* h, unsigned short** dst3, unsigned short** dst2, const float* src, int batch, long long s_src, int N, int K,
               int ld, float wscale) {
  unsigned short** dst[2] = {dst3, dst2};
  for (int i = 0; i < 2; i++) {
    const MlpArith ar = planes_arith(i);
    const size_t elems = split_elems(N, K, ar) * (size_t)batch;
    HIP_TRY(h, hipMalloc((void**)dst[i], std::max<size_t>(elems, 1) * sizeof(unsigned short)));
    launch_split_planes(src, batch, s_src, N, K, ld, ar, wscale, *dst[i], nullptr);
  }
  HIP_TRY(h, hipDeviceSynchronize());
  return ANI_OK;
}

int upload_model(ani_handle* h) {
  const HostModel& m = h->model;
  const int L = m.L, M = m.M;
  const int aev_stride = round_up(m.aev_len, 4);
  h->nets.resize(m.S);
  for (int s = 0; s < m.S; s++) {
    SpeciesNet& n = h->nets[s];
    const std::vector<int>& d = m.dims[s];
    n.w.resize(L);
    n.w[0] = aev_stride;
    for (int k = 1; k < L; k++) n.w[k] = round_up(d[k], 4);
    if (d[L - 1] > 256) { h->err = "last hidden layer wider than 256 is not supported"; return ANI_ERR_MODEL; }
    n.W.assign(L - 1, nullptr); n.b.assign(L - 1, nullptr); n.WT.assign(L - 1, nullptr);
    n.W64.assign(L - 1, nullptr); n.b64.assign(L - 1, nullptr); n.WT64.assign(L - 1, nullptr);
    for (auto& sp : n.sp) { sp.W.assign(L - 1, nullptr); sp.WT.assign(L - 1, nullptr); }
    n.wscale.assign(L - 1, 1.f);
    for (int k = 0; k < L - 1; k++) {
      const int out = d[k + 1], in = d[k], kp = n.w[k];
      float wmax = 0.f;
      for (int a = 0; a < M; a++)
        for (float v : m.W[a][s][k]) wmax = std::max(wmax, std::fabs(v));
      if (!std::isfinite(wmax)) { h->err = "non-finite weight in the model file"; return ANI_ERR_MODEL; }
      int e = 0;
      if (wmax > 0.f) (void)std::frexp(wmax, &e);   // wmax = f * 2^e, f in [0.5, 1)
      n.wscale[k] = std::ldexp(1.f, std::max(-24, std::min(24, 13 - e)));
      std::vector<float> W((size_t)M * out * kp, 0.f), b((size_t)M * out);
      for (int a = 0; a < M; a++) {
        for (int o = 0; o < out; o++) {
          memcpy(&W[((size_t)a * out + o) * kp], &m.W[a][s][k][(size_t)o * in], sizeof(float) * in);
          b[(size_t)a * out + o] = m.b[a][s][k][o];
        }
      }
      int rc = upload(h, &n.W[k], W); if (rc) return rc;
      rc = upload(h, &n.b[k], b); if (rc) return rc;
      rc = mirror64(h, &n.W64[k], n.W[k], W.size()); if (rc) return rc;
      rc = mirror64(h, &n.b64[k], n.b[k], b.size()); if (rc) return rc;
      rc = make_split(h, &n.sp[0].W[k], &n.sp[1].W[k], n.W[k], M, (long long)out * kp, out, kp, kp, n.wscale[k]); if (rc) return rc;
      // transposed copies for the backward products
      if (k == 0) {
        const int w1 = n.w[1];
        std::vector<float> T((size_t)m.aev_len * M * w1, 0.f);   // [aev_len][M*w1]
        for (int a = 0; a < M; a++)
          for (int o = 0; o < out; o++)
            for (int i = 0; i < in; i++) T[(size_t)i * M * w1 + (size_t)a * w1 + o] = m.W[a][s][0][(size_t)o * in + i];
        rc = upload(h, &n.WT[0], T); if (rc) return rc;
        rc = mirror64(h, &n.WT64[0], n.WT[0], T.size()); if (rc) return rc;
        rc = make_split(h, &n.sp[0].WT[0], &n.sp[1].WT[0], n.WT[0], 1, 0, m.aev_len, M * w1, M * w1, n.wscale[0]); if (rc) return rc;
      } else {
        const int wk1 = n.w[k + 1 < L ? k + 1 : k];  // K of the backward product through layer k = padded d[k+1]
        std::vector<float> T((size_t)M * in * wk1, 0.f);         // [M][d[k]][w(k+1)]
        for (int a = 0; a < M; a++)
          for (int o = 0; o < out; o++)
            for (int i = 0; i < in; i++) T[((size_t)a * in + i) * wk1 + o] = m.W[a][s][k][(size_t)o * in + i];
        rc = upload(h, &n.WT[k], T); if (rc) return rc;
        rc = mirror64(h, &n.WT64[k], n.WT[k], T.size()); if (rc) return rc;
        rc = make_split(h, &n.sp[0].WT[k], &n.sp[1].WT[k], n.WT[k], M, (long long)in * wk1, in, wk1, wk1, n.wscale[k]); if (rc) return rc;
      }
    }
    {  // output layer
      const int in = d[L - 1], kp = n.w[L - 1];
      std::vector<float> w((size_t)M * kp, 0.f), b(M);
      for (int a = 0; a < M; a++) {
        memcpy(&w[(size_t)a * kp], m.W[a][s][L - 1].data(), sizeof(float) * in);
        b[a] = m.b[a][s][L - 1][0];
      }
      int rc = upload(h, &n.w_out, w); if (rc) return rc;
      rc = upload(h, &n.b_out, b); if (rc) return rc;
      rc = mirror64(h, &n.w_out64, n.w_out, w.size()); if (rc) return rc;
      rc = mirror64(h, &n.b_out64, n.b_out, b.size()); if (rc) return rc;
    }
  }
  if (m.has_rep) {
    HIP_TRY(h, h->rep_tables.reserve(m.rep_tables.size()));
    HIP_TRY(h, hipMemcpy(h->rep_tables.p, m.rep_tables.data(), sizeof(double) * m.rep_tables.size(), hipMemcpyHostToDevice));
  }
  AevParams& p = h->ap;
  memset(&p, 0, sizeof(p));
  p.S = m.S; p.nR = m.nR; p.nA = m.nA; p.nZ = m.nZ; p.nAZ = m.nA * m.nZ;
  p.radial_len = m.radial_len; p.aev_len = m.aev_len; p.aev_stride = aev_stride;
  p.compat = h->use_cuaev ? 0 : 1;
  p.full_cap = 0;
  p.Rcr = (float)m.Rcr; p.Rca = (float)m.Rca; p.EtaR = (float)m.EtaR; p.EtaA = (float)m.EtaA; p.Zeta = (float)m.Zeta;
  p.pi_over_Rcr = (float)(M_PI / m.Rcr); p.pi_over_Rca = (float)(M_PI / m.Rca);
  for (int k = 0; k < m.nR; k++) p.ShfR[k] = (float)m.ShfR[k];
  for (int k = 0; k < m.nA; k++) p.ShfA[k] = (float)m.ShfA[k];
  for (int k = 0; k < m.nZ; k++) { p.cosZ[k] = (float)cos(m.ShfZ[k]); p.sinZ[k] = (float)sin(m.ShfZ[k]); }
  {
    const double dR = m.nR > 1 ? (m.ShfR[m.nR - 1] - m.ShfR[0]) / (m.nR - 1) : 0.0;
    const double dA = m.nA > 1 ? (m.ShfA[m.nA - 1] - m.ShfA[0]) / (m.nA - 1) : 0.0;
    bool equi = true;
    for (int k = 0; k < m.nR; k++) equi = equi && std::fabs(m.ShfR[0] + k * dR - m.ShfR[k]) < 1e-9;
    for (int k = 0; k < m.nA; k++) equi = equi && std::fabs(m.ShfA[0] + k * dA - m.ShfA[k]) < 1e-9;
    p.ShfR0 = (float)m.ShfR[0]; p.dShfR = (float)dR; p.ShfA0 = (float)m.ShfA[0]; p.dShfA = (float)dA;
    p.equi = equi ? 1 : 0;
  }
  if (aev_stride > 1024) { h->err = "AEV longer than 1024 is not supported"; return ANI_ERR_MODEL; }
  return ANI_OK;
}

// AEV columns of species that do not occur in the system (centres or neighbours) are identically zero, so the
// first-layer products only need the columns of the species present: exact same sums with the zero terms left out.
// The AEV kernels then run with a compact layout (S' species, A' = 16 S' + 32 S'(S'+1)/2 columns) and the first layer /
// dE/dAEV products use column-gathered weights.  Water with ANI-2x: 1008 -> 128 columns; C,H,N,O systems: 384.
int specialize(ani_handle* h, int mask) {
  const HostModel& m = h->model;
  if (!h->opt.prune) mask = (1 << m.S) - 1;
  if (mask == h->active_mask) return ANI_OK;
  for (auto& n : h->nets) {
    if (n.W0c) (void)hipFree(n.W0c);
    if (n.WT0c) (void)hipFree(n.WT0c);
    if (n.W0c64) (void)hipFree(n.W0c64);
    if (n.WT0c64) (void)hipFree(n.WT0c64);
    for (auto& sp : n.sp) {
      if (sp.W0c) (void)hipFree(sp.W0c);
      if (sp.WT0c) (void)hipFree(sp.WT0c);
      sp.W0c = sp.WT0c = nullptr;
    }
    n.W0c = n.WT0c = nullptr;
    n.W0c64 = n.WT0c64 = nullptr;
  }
  std::vector<int> act;
  for (int s = 0; s < m.S; s++) {
    h->cmap.m[s] = (int)act.size();
    if (mask & (1 << s)) act.push_back(s);
  }
  for (int s = m.S; s < kMaxSpecies; s++) h->cmap.m[s] = 0;
  const int na = (int)act.size();
  h->ap_run = h->ap;
  h->colmap.resize(m.aev_len);
  for (int c = 0; c < m.aev_len; c++) h->colmap[c] = c;
  h->active_mask = mask;
  if (na == m.S || na == 0) {
    for (int s = 0; s < m.S; s++) h->cmap.m[s] = s;
    return ANI_OK;
  }
  const int nAZ = m.nA * m.nZ;
  const int alen = na * m.nR + na * (na + 1) / 2 * nAZ;
  const int astride = round_up(alen, 4);
  AevParams& p = h->ap_run;
  p.S = na; p.radial_len = na * m.nR; p.aev_len = alen; p.aev_stride = astride;
  h->colmap.assign(alen, 0);
  for (int cs = 0; cs < na; cs++)
    for (int k = 0; k < m.nR; k++) h->colmap[cs * m.nR + k] = act[cs] * m.nR + k;
  {
    int b = 0;
    for (int c1 = 0; c1 < na; c1++)
      for (int c2 = c1; c2 < na; c2++, b++) {
        const int lo = act[c1], hi = act[c2];
        const int dense_b = lo * m.S - lo * (lo - 1) / 2 + (hi - lo);
        for (int t = 0; t < nAZ; t++) h->colmap[na * m.nR + b * nAZ + t] = m.radial_len + dense_b * nAZ + t;
      }
  }
  const int M = m.M;
  for (int s = 0; s < m.S; s++) {
    SpeciesNet& n = h->nets[s];
    const int out = m.dims[s][1], in = m.dims[s][0], w1 = n.w[1];
    std::vector<float> W((size_t)M * out * astride, 0.f), T((size_t)alen * M * w1, 0.f);
    for (int a = 0; a < M; a++)
      for (int o = 0; o < out; o++)
        for (int c = 0; c < alen; c++) {
          const float v = m.W[a][s][0][(size_t)o * in + h->colmap[c]];
          W[((size_t)a * out + o) * astride + c] = v;
          T[(size_t)c * M * w1 + (size_t)a * w1 + o] = v;
        }
    int rc = upload(h, &n.W0c, W); if (rc) return rc;
    rc = upload(h, &n.WT0c, T); if (rc) return rc;
    rc = mirror64(h, &n.W0c64, n.W0c, W.size()); if (rc) return rc;
    rc = mirror64(h, &n.WT0c64, n.WT0c, T.size()); if (rc) return rc;
    rc = make_split(h, &n.sp[0].W0c, &n.sp[1].W0c, n.W0c, M, (long long)out * astride, out, astride, astride, n.wscale[0]); if (rc) return rc;
    rc = make_split(h, &n.sp[0].WT0c, &n.sp[1].WT0c, n.WT0c, 1, 0, alen, M * w1, M * w1, n.wscale[0]); if (rc) return rc;
  }
  return ANI_OK;
}

// Stream tables of the AEV kernels for the species map just installed (StreamTab in ani_kernels.h): built once per map -- a
// re-neighbouring with the same species present returns at the first test.  Two passes per table: the lengths of every tuple's
// stream (the kernels' own table builders on the device), an exclusive sum on the host, then the words.  A layout of three or more
// species, or a shape off the fast path, has none.  The S = 2 bound is halved until both tables fit kStreamTabMaxBytes.
int build_stream_tables(ani_handle* h, hipStream_t st) {
  StreamTables& t = h->stab;
  if (t.mask == h->active_mask) return ANI_OK;
  const auto t0 = std::chrono::steady_clock::now();
  t.mask = h->active_mask;
  t.S = 0; t.nt = 0; t.tuples = 0; t.nwords_b = t.nwords_f = 0;
  const AevParams& p = h->ap_run;
  if (!h->use_single || !stream_tab_supported(p)) return ANI_OK;
  std::vector<int4> db, df;
  for (int nt = p.S == 1 ? kMaxAng : kStreamTabNT; nt >= 1; nt /= 2) {
    const int n = stream_tab_tuples(p.S, nt);
    HIP_TRY(h, t.desc_b.reserve(n));
    HIP_TRY(h, t.desc_f.reserve(n));
    launch_stream_table(p, nt, true, t.desc_b.p, nullptr, 0, st);
    launch_stream_table(p, nt, false, t.desc_f.p, nullptr, 0, st);
    db.resize(n); df.resize(n);
    HIP_TRY(h, hipMemcpyAsync(db.data(), t.desc_b.p, sizeof(int4) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(df.data(), t.desc_f.p, sizeof(int4) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    size_t nb = 0, nf = 0;
    for (int i = 0; i < n; i++) { db[i].x = (int)nb; nb += db[i].w; df[i].x = (int)nf; nf += df[i].w; }
    if ((nb + nf) * sizeof(unsigned) + 2 * sizeof(int4) * (size_t)n > kStreamTabMaxBytes) continue;
    HIP_TRY(h, t.words_b.reserve(std::max<size_t>(nb, 1)));
    HIP_TRY(h, t.words_f.reserve(std::max<size_t>(nf, 1)));
    HIP_TRY(h, hipMemcpyAsync(t.desc_b.p, db.data(), sizeof(int4) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t.desc_f.p, df.data(), sizeof(int4) * n, hipMemcpyHostToDevice, st));
    launch_stream_table(p, nt, true, t.desc_b.p, t.words_b.p, 1, st);
    launch_stream_table(p, nt, false, t.desc_f.p, t.words_f.p, 1, st);
    HIP_TRY(h, hipStreamSynchronize(st));   // db / df leave scope; the build is timed whole
    HIP_TRY(h, hipGetLastError());
    t.S = p.S; t.nt = nt; t.tuples = n; t.nwords_b = nb; t.nwords_f = nf;
    break;
  }
  t.builds++;
  t.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ANI_OK;
}
}  // namespace ani_host
