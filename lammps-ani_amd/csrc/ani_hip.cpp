// ani_hip.cpp — C ABI of libani_hip.so (include/ani_hip.h), replacing class ANI of the reference (src/ani_csrc/ani.cpp) without
// libtorch: create / destroy, the per-step pipeline, the whole-step and split-step entry points.  The handle is in ani_handle.h; beside
// this file ani_hip_{model,mlp,list,armed,analysis,options}.cpp: weights, MLP host side, list epoch, per-call armings, analysis, options.
// Per step (all on one HIP stream, no per-step allocation once buffers have grown):
//   [ago==0 only]  upload / copy the neighbour list, scan numneigh, bucket the centres by species (rows padded to
//                  128 per species so that every GEMM tile is species-pure)            (ani.cpp:213-229)
//   pack           double positions -> float4 {x,y,z,species}                          (ani.cpp:206-209)
//   AEV forward    -> aev[nrows][aev_stride], rows in species-bucket order             (lammps_ani.py:174)
//   MLP            forward + input-gradient backward on MFMA (fp32 products as six bf16 terms, or fp32-input MFMA) -> e_rows, gaev      (lammps_ani.py:182-184,197)
//   AEV backward   gaev -> forces on local+ghost atoms, virial                         (lammps_ani.py:195-216)
//   finish         fp64 energy sum + self energies, kcal/mol conversion                (ani.cpp:246-262)
#include "ani_handle.h"

namespace ani {
static thread_local hipError_t g_launch_error = hipSuccess;
void note_launch_error(hipError_t e) { if (e != hipSuccess && g_launch_error == hipSuccess) g_launch_error = e; }
hipError_t take_launch_error() { const hipError_t e = g_launch_error; g_launch_error = hipSuccess; return e; }
}  // namespace ani

namespace ani_host __attribute__((visibility("hidden"))) {
thread_local std::string g_create_error;
constexpr int kCopyOutBlocks = 32;   // workgroups of launch_copy_out: enough stores in flight for the link, few enough to finish chunks in order

// precision 'double': same pipeline on the fp64 kernels (ani_kernels_f64.hip)
int run_step64(ani_handle* h, const double* d_x, int eflag_atom, int vflag, double* d_f, int f_accumulate, double* d_ev,
               double* d_eatom, hipStream_t st) {
  const HostModel& m = h->model;
  const int L = m.L, M = m.M;
  HIP_TRY(h, h->fbuf64.reserve((size_t)std::max(h->ntotal, 1) * 3));
  HIP_TRY(h, h->virial_acc.reserve(9 * kVirialSlots));
  HIP_TRY(h, h->err_flag.reserve(1, true));
  HIP_TRY(h, hipMemsetAsync(h->fbuf64.p, 0, sizeof(double) * 3 * (size_t)h->ntotal, st));
  HIP_TRY(h, hipMemsetAsync(h->virial_acc.p, 0, sizeof(double) * 9, st));
  HIP_TRY(h, hipMemsetAsync(h->e_rows64.p, 0, sizeof(double) * (size_t)M * std::max(h->nrows, 1), st));
  if (h->armed.av_acc) HIP_TRY(h, hipMemsetAsync(h->armed.av_acc, 0, sizeof(double) * 9 * (size_t)h->ntotal, st));
  Aev64Params p{};
  const AevParams& r = h->ap_run;
  p.S = r.S; p.nR = r.nR; p.nA = r.nA; p.nZ = r.nZ; p.radial_len = r.radial_len; p.aev_len = r.aev_len; p.aev_stride = r.aev_stride;
  p.compat = r.compat;
  p.Rcr = m.Rcr; p.Rca = m.Rca; p.EtaR = m.EtaR; p.EtaA = m.EtaA; p.Zeta = m.Zeta;
  for (int k = 0; k < m.nR; k++) p.ShfR[k] = m.ShfR[k];
  for (int k = 0; k < m.nA; k++) p.ShfA[k] = m.ShfA[k];
  for (int k = 0; k < m.nZ; k++) { p.cosZ[k] = cos(m.ShfZ[k]); p.sinZ[k] = sin(m.ShfZ[k]); }
  Aev64Args a{};
  a.x = d_x; a.species = h->species.p; a.cmap = h->cmap; a.jlist = h->jlist.p; a.row_info = h->row_info.p; a.nrows = h->nrows;
  a.aev = h->aev64.p; a.gaev = h->gaev64.p; a.fbuf = h->fbuf64.p; a.virial = vflag ? h->virial_acc.p : nullptr;
  a.err_flag = h->err_flag.p;
  launch_aev64_forward(p, a, st);
  const int ka = r.aev_stride;
  const size_t per = (size_t)std::max(h->nrows, 1) * ka;   // model-deviation step: rows of a member in gaev_parts64
  if (h->armed.dv_force) HIP_TRY(h, h->armed.gaev_parts64.reserve(per * M, true));
  for (int s = 0; s < m.S; s++) {
    if (h->count[s] == 0) continue;
    const SpeciesNet& n = h->nets[s];
    const std::vector<int>& d = m.dims[s];
    const int rows = round_up(h->count[s], kRowTile), r0 = h->row_start[s];
    auto base = [&]() {
      Gemm64Args g{};
      g.rows = rows; g.batch = M; g.alpha = m.alpha; g.scale = 1.0 / M; g.centre_of_row = h->centre_of_row.p + r0;
      return g;
    };
    for (int k = 0; k <= L - 2; k++) {
      Gemm64Args g = base();
      if (k == 0) {
        g.A = h->aev64.p + (size_t)r0 * ka; g.lda = ka; g.sA = 0; g.K = ka;
        g.Bt = n.W0c64 ? n.W0c64 : n.W64[0]; g.ldb = ka; g.sB = (long long)d[1] * ka;
      } else {
        g.A = h->Hbuf64[s][k]; g.lda = M * n.w[k]; g.sA = n.w[k]; g.K = n.w[k];
        g.Bt = n.W64[k]; g.ldb = n.w[k]; g.sB = (long long)d[k + 1] * n.w[k];
      }
      g.N = d[k + 1]; g.bias = n.b64[k]; g.sBias = d[k + 1];
      g.C = h->Hbuf64[s][k + 1]; g.ldc = M * n.w[k + 1]; g.sC = n.w[k + 1];
      if (k == L - 2) {
        g.aux = n.w_out64; g.sAux = n.w[L - 1]; g.bias_last = n.b_out64;
        g.e_out = h->e_rows64.p + r0; g.sE = h->nrows;
      }
      launch_gemm64(g, k == L - 2 ? EPI_LAST : EPI_CELU, st);
    }
    for (int k = L - 1; k >= 2; k--) {
      Gemm64Args g = base();
      g.A = h->Hbuf64[s][k]; g.lda = M * n.w[k]; g.sA = n.w[k]; g.K = n.w[k];
      g.Bt = n.WT64[k - 1]; g.ldb = n.w[k]; g.sB = (long long)d[k - 1] * n.w[k];
      g.N = d[k - 1];
      g.aux = h->Hbuf64[s][k - 1]; g.ldaux = M * n.w[k - 1]; g.sAux = n.w[k - 1];
      g.C = h->Hbuf64[s][k - 1]; g.ldc = M * n.w[k - 1]; g.sC = n.w[k - 1];
      launch_gemm64(g, EPI_BWD, st);
    }
    {
      Gemm64Args g = base();
      g.batch = 1;
      g.A = h->Hbuf64[s][1]; g.lda = M * n.w[1]; g.K = M * n.w[1];
      g.Bt = n.WT0c64 ? n.WT0c64 : n.WT64[0]; g.ldb = M * n.w[1];
      g.N = r.aev_len;
      g.C = h->gaev64.p + (size_t)r0 * ka; g.ldc = ka;
      launch_gemm64(g, EPI_PLAIN, st);
    }
    if (h->armed.dv_force) {   // every member's own rows: G_1 of member b (columns b w[1]) times its slice of WT[0]
      Gemm64Args g = base();
      g.A = h->Hbuf64[s][1]; g.lda = M * n.w[1]; g.sA = n.w[1]; g.K = n.w[1];
      g.Bt = n.WT0c64 ? n.WT0c64 : n.WT64[0]; g.ldb = M * n.w[1]; g.sB = n.w[1];
      g.N = r.aev_len;
      g.C = h->armed.gaev_parts64.p + (size_t)r0 * ka; g.ldc = ka; g.sC = (long long)per;
      launch_gemm64(g, EPI_PLAIN, st);
    }
  }
  if (h->armed.dv_force) launch_dev_parts64(h->armed.gaev_parts64.p, (long long)per, M, h->gaev64.p, (long long)h->nrows * ka, st);
  launch_aev64_backward(p, a, st, static_cast<double*>(h->armed.av_acc));
  if (m.has_rep) {
    HIP_TRY(h, h->erep.reserve(kVirialSlots));
    HIP_TRY(h, hipMemsetAsync(h->erep.p, 0, sizeof(double) * kVirialSlots, st));
    RepArgs ra{};
    ra.row_info = h->row_info.p; ra.nrows = h->nrows; ra.jlist = h->jlist.p; ra.species = h->species.p;
    ra.pos = d_x; ra.fbuf = h->fbuf64.p; ra.virial = vflag ? h->virial_acc.p : nullptr; ra.erep = h->erep.p;
    ra.tables = h->rep_tables.p; ra.S = m.S; ra.nslots = kVirialSlots; ra.vslots = 1; ra.cutoff = m.rep_cut;
    launch_repulsion(ra, true, st, h->armed.av_acc);
    h->last_rep_kernel = "repulsion_kernel<double>";
  }
  Sae64 sae{};
  for (int s = 0; s < m.S; s++) sae.v[s] = m.sae[s];
  launch_finish64(h->e_rows64.p, M, h->nrows, h->centre_of_row.p, h->ilist.p, h->species.p, sae, h->fbuf64.p, h->ntotal,
                  vflag ? h->virial_acc.p : nullptr, d_f, f_accumulate, d_ev, eflag_atom ? d_eatom : nullptr, h->err_flag.p, st);
  if (m.has_rep) launch_repulsion_energy(h->erep.p, kVirialSlots, d_ev, st);
  if (h->armed.dv_on) {
    Aev64Args ad = a;
    ad.virial = nullptr;
    const int rcd = deviation_run(h, [&](int b, long long stride, void* acc) {
      ad.gaev = h->armed.gaev_parts64.p + b * stride; ad.fbuf = static_cast<double*>(acc);
      launch_aev64_backward(p, ad, st);
    }, st);
    if (rcd) return rcd;
  }
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, take_launch_error());
  return ANI_OK;
}

// the per-step pipeline on device-resident inputs; the list of this epoch is already in the handle's buffers
// ---- one step of the fp32 pipeline, in pieces: a whole step (run_step) strings them together on one stream; the split
// entry points (ani_step_begin / ani_step_ghosts_ready / ani_step_finish) cut it where the ghost exchange happens ----
struct StepCtx {
  const double* d_x = nullptr;
  int eflag_atom = 0, vflag = 0, f_accumulate = 0;
  double *d_f = nullptr, *d_ev = nullptr, *d_eatom = nullptr;
  bool fold = false;   // whole-step device call: an installed ghost fold applies (pack gathers the images, finish folds their forces)
};

int step_prologue(ani_handle* h, const StepCtx& c, bool timed, hipStream_t st) {
  if (h->ntotal >= (1 << 28)) {   // the compact lists keep an atom index in 28 bits (AevArgs::cl_j)
    h->err = "more than 2^28 atoms (owned + ghost) on one rank";
    return ANI_ERR_ARG;
  }
  HIP_TRY(h, h->xyzs.reserve(h->ntotal));
  HIP_TRY(h, h->fbuf.reserve((size_t)h->ntotal * 4));  // one float4 per atom
  HIP_TRY(h, h->virial_acc.reserve(9 * kVirialSlots));
  HIP_TRY(h, h->err_flag.reserve(1, true));
  HIP_TRY(h, h->row_ctr.reserve((size_t)3 * kTicketMaxGroups * kTicketStride, true));
  h->timing.evt = nullptr;
  if (timed && h->timing.on) {
    if (h->timing.evt_used + 6 > h->timing.evt_pool.size()) {
      const size_t old = h->timing.evt_pool.size();
      h->timing.evt_pool.resize(old + 6 * 64, nullptr);
      for (size_t i = old; i < h->timing.evt_pool.size(); i++) HIP_TRY(h, hipEventCreate(&h->timing.evt_pool[i]));
    }
    h->timing.evt = &h->timing.evt_pool[h->timing.evt_used];
    h->timing.evt_used += 6;
  }
  if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[0], st));
  HIP_TRY(h, h->origin.reserve(3));
  if (h->need_origin) {
    launch_origin(c.d_x, h->ntotal, h->origin.p, st);
    h->need_origin = false;
  }
  if (h->model.has_rep) {
    HIP_TRY(h, h->erep.reserve(kVirialSlots));
    HIP_TRY(h, hipMemsetAsync(h->erep.p, 0, sizeof(double) * kVirialSlots, st));
  }
  return ANI_OK;
}

// atoms [i0, i1) -> fp32 positions, force accumulators cleared; `first`: also the step's virial / energy accumulators
void step_pack(ani_handle* h, const StepCtx& c, int i0, int i1, bool first, hipStream_t st) {
  const bool fold = h->fold_nghost >= 0 && c.fold;
  launch_pack(c.d_x, h->species.p, i0, i1, h->cmap, h->xyzs.p, h->fbuf.p, first ? h->virial_acc.p : nullptr,
              first ? c.d_ev : nullptr, h->origin.p, st, fold ? &h->fold : nullptr);
}

// rows: 0 = every row, 1 = the rows with a ghost among their candidates, 2 = the others (fast path only)
AevArgs step_aev_args(ani_handle* h, const StepCtx& c, int rows) {
  AevArgs a{};
  a.xyzs = h->xyzs.p; a.ilist = h->ilist.p; a.numneigh = h->numneigh.p; a.nbr_off = h->nbr_off.p; a.jlist = h->jlist.p;
  a.centre_of_row = h->centre_of_row.p; a.row_info = h->row_info.p; a.nrows = h->nrows; a.aev = h->aev.p; a.gaev = h->gaev.p; a.fbuf = h->fbuf.p;
  a.virial = c.vflag ? h->virial_acc.p : nullptr;
  a.err_flag = h->err_flag.p;
  a.cl_hdr = h->cl_hdr.p; a.cl_xyz = h->cl_xyz.p; a.cl_j = h->cl_j.p; a.cl_stride = h->cl_stride;
  a.row_list = nullptr; a.k0 = 0; a.kcount = h->nrows;
  a.row_counter = h->row_ctr.p ? h->row_ctr.p + rows * kTicketMaxGroups * kTicketStride : nullptr;
  if (rows == 1) { a.row_list = h->row_list.p; a.k0 = 0; a.kcount = h->n_boundary; }
  if (rows == 2) { a.row_list = h->row_list.p; a.k0 = h->n_boundary; a.kcount = h->nrows - h->n_boundary; }
  // rows by ticket pay from a few rows per wave on (the ~5000 resident waves of a launch each draw three tickets before their
  // first centre): below that the fixed stride is as good and starts at once (option "aev_tickets_min")
  if (a.kcount < h->opt.aev_tickets_min) a.row_counter = nullptr;
  // a centre may read its neighbours' dE/dAEV rows only when every row of the step has been through the MLP: not in a split step
  a.row_of_atom = (rows == 0 && h->opt.aev_sym_radial && h->list_symmetric) ? h->row_of_atom.p : nullptr;
  return a;
}

// the handle's stream tables for a launch; NULL: arithmetic slot decode (option off, or no tables for the layout of the epoch)
static const StreamTab* step_stream_tab(const ani_handle* h, StreamTab& view) {
  if (!h->opt.aev_stream_tables || h->stab.S == 0 || h->stab.S != h->ap_run.S || h->stab.mask != h->active_mask) return nullptr;
  view = h->stab.view();
  return &view;
}

int step_compact_forward(ani_handle* h, const AevArgs& a, hipStream_t st) {
  StreamTab tab_view;
  const StreamTab* tab = step_stream_tab(h, tab_view);
  if (h->opt.aev_fused) {
    TraceRange tr("ani: neighbour compaction + AEV forward");
    if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[5], st));   // the compaction phase is inside the forward launch
    if (launch_aev_forward_fused(h->ap_run, a, h->max_numneigh, st, tab)) {
      if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[1], st));
      return ANI_OK;
    }
  }
  {
    TraceRange tr("ani: neighbour compaction");
    launch_nbr_compact(h->ap_run, a, h->max_numneigh, st);
  }
  if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[5], st));
  {
    TraceRange tr("ani: AEV forward");
    launch_aev_forward(h->ap_run, a, h->max_numneigh, st, tab);
  }
  if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[1], st));
  return ANI_OK;
}

// The repulsion is folded into the radial stage of the fast AEV backward kernel: at most 8 species present (its tables), and
// every pair inside the block's cutoff among the entries that stage walks -- the compacted radial list holds r <= Rcr, so
// rep_cut <= Rcr, or the pyaev mode, which keeps every candidate.  Otherwise the stand-alone kernel adds the term.
bool rep_folded(const ani_handle* h) {
  const HostModel& m = h->model;
  return m.has_rep && h->ap_run.S <= 8 && (m.rep_cut <= m.Rcr || h->ap_run.compat);
}

int step_backward(ani_handle* h, const StepCtx& c, const AevArgs& a, hipStream_t st) {
  const HostModel& m = h->model;
  // the fast backward kernel applies the repulsion in its radial stage (tables by compact species, like the AEV layout);
  // the generic kernel does not, and then the stand-alone kernel adds it
  RepTab rt{};
  if (rep_folded(h)) {
    rt.on = 1; rt.cutoff = (float)m.rep_cut; rt.erep = h->erep.p; rt.x64 = c.d_x;
    std::vector<int> act;
    for (int s = 0; s < m.S; s++) if (h->active_mask & (1 << s)) act.push_back(s);
    if ((int)act.size() != h->ap_run.S) { act.clear(); for (int s = 0; s < m.S; s++) act.push_back(s); }
    const size_t n2 = (size_t)m.S * m.S;
    for (size_t ca = 0; ca < act.size(); ca++)
      for (size_t cb = 0; cb < act.size(); cb++) {
        const size_t src = (size_t)act[ca] * m.S + act[cb];
        rt.y[8 * ca + cb] = (float)m.rep_tables[src];
        rt.sa[8 * ca + cb] = (float)m.rep_tables[n2 + src];
        rt.k[8 * ca + cb] = (float)m.rep_tables[2 * n2 + src];
      }
  }
  float* avir = static_cast<float*>(h->armed.av_acc);   // armed step: per-atom virial (ani_request_atom_virial)
  StreamTab tab_view;
  const bool rep_done = launch_aev_backward(h->ap_run, a, h->max_numneigh, st, rt.on ? &rt : nullptr, avir, step_stream_tab(h, tab_view)) && rt.on;
  if (m.has_rep) h->last_rep_kernel = rep_done ? "aev_backward_fast" : "repulsion_kernel<float>";
  if (m.has_rep && !rep_done) {
    RepArgs ra{};
    ra.row_info = h->row_info.p; ra.nrows = h->nrows; ra.jlist = h->jlist.p; ra.species = h->species.p;
    ra.pos = c.d_x; ra.fbuf = h->fbuf.p; ra.virial = c.vflag ? h->virial_acc.p : nullptr; ra.erep = h->erep.p;
    ra.tables = h->rep_tables.p; ra.S = m.S; ra.nslots = kVirialSlots; ra.vslots = kVirialSlots; ra.cutoff = m.rep_cut;
    launch_repulsion(ra, false, st, avir);
  }
  return ANI_OK;
}

// forces of the atoms [atom0, atom1) leave the accumulators; `energy`: also the step's energy / virial / repulsion energy
void step_finish(ani_handle* h, const StepCtx& c, int atom0, int atom1, bool energy, hipStream_t st) {
  const HostModel& m = h->model;
  FinishArgs fa{};
  fa.e_rows = h->e_rows.p; fa.M = m.M; fa.nrows = h->nrows; fa.nrows_ld = h->nrows;
  fa.centre_of_row = h->centre_of_row.p; fa.ilist = h->ilist.p; fa.species = h->species.p;
  for (int s = 0; s < m.S; s++) fa.sae[s] = m.sae[s];
  fa.fbuf = h->fbuf.p; fa.atom0 = atom0; fa.atom1 = atom1; fa.energy = energy ? 1 : 0;
  fa.virial_acc = c.vflag ? h->virial_acc.p : nullptr;
  fa.f_out = c.d_f; fa.f_accumulate = c.f_accumulate; fa.ev_out = c.d_ev;
  fa.eatom_out = c.eflag_atom ? c.d_eatom : nullptr;
  fa.err_flag = h->err_flag.p;
  if (h->fold_nghost >= 0 && c.fold) {
    fa.fold_head = h->fold_head.p; fa.fold_next = h->fold_next.p; fa.fold_nlocal = h->nlocal;
    fa.atom1 = std::min(fa.atom1, h->nlocal);   // the ghost rows of d_f are not written: their forces went home
  }
  launch_finish(fa, st);
  if (energy && m.has_rep) launch_repulsion_energy(h->erep.p, kVirialSlots, c.d_ev, st);
}

int run_step(ani_handle* h, const double* d_x, int eflag_atom, int vflag, double* d_f, int f_accumulate, double* d_ev,
             double* d_eatom, hipStream_t st, bool fold = false) {
  if (!h->use_single) return run_step64(h, d_x, eflag_atom, vflag, d_f, f_accumulate, d_ev, d_eatom, st);
  StepCtx c;
  c.fold = fold;
  c.d_x = d_x; c.eflag_atom = eflag_atom; c.vflag = vflag; c.f_accumulate = f_accumulate; c.d_f = d_f; c.d_ev = d_ev; c.d_eatom = d_eatom;
  TraceRange tr_step("ani: step");
  int rc = step_prologue(h, c, true, st);
  if (rc) return rc;
  step_pack(h, c, 0, h->ntotal, true, st);   // also clears fbuf / virial_acc / the energy word
  if (h->armed.av_acc) HIP_TRY(h, hipMemsetAsync(h->armed.av_acc, 0, sizeof(float) * 9 * (size_t)h->ntotal, st));
  const AevArgs a = step_aev_args(h, c, 0);
  rc = step_compact_forward(h, a, st);
  if (rc) return rc;
  {
    TraceRange tr("ani: MLP forward + backward");
    rc = compute_mlp(h, st);
    if (rc) return rc;
  }
  if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[2], st));
  TraceRange tr_bwd("ani: AEV backward + finish");
  rc = step_backward(h, c, a, st);
  if (rc) return rc;
  if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[3], st));
  step_finish(h, c, 0, h->ntotal, true, st);
  if (h->timing.evt) HIP_TRY(h, hipEventRecord(h->timing.evt[4], st));
  if (h->armed.dv_on) {
    AevArgs ad = a;
    ad.virial = nullptr;
    rc = deviation_run(h, [&](int b, long long stride, void* acc) {
      ad.gaev = h->fused.gaev_parts.p + b * stride; ad.fbuf = static_cast<float*>(acc);
      launch_aev_backward(h->ap_run, ad, h->max_numneigh, st);
    }, st);
    if (rc) return rc;
  }
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, take_launch_error());
  return ANI_OK;
}

bool split_supported(const ani_handle* h) { return h->use_single && h->cl_stride > 0 && (!h->model.has_rep || rep_folded(h)); }

int check_args(ani_handle* h, int ntotal, int nlocal, long long npairs, int ago) {
  if (!h) return ANI_ERR_ARG;
  if (ntotal < 0 || nlocal < 0 || nlocal > ntotal || npairs < 0) { h->err = "inconsistent ntotal/nlocal/npairs"; return ANI_ERR_ARG; }
  if (npairs >= (1LL << 31)) { h->err = "more than 2^31 neighbour pairs per rank is not supported"; return ANI_ERR_ARG; }
  if (ago != 0 && (!h->have_list || ntotal != h->ntotal || nlocal != h->nlocal)) {
    h->err = "ago != 0 but no neighbour list of matching size is cached (the first call, and every call after a rebuild, must pass ago = 0)";
    return ANI_ERR_ARG;
  }
  return ANI_OK;
}

int finish_host(ani_handle* h, int ntotal, int nlocal, int eflag_atom, int vflag, double* out_energy, double* out_force,
                double* out_atomic_energies, double* out_virial) {
  hipStream_t st = h->stream;
  if (!h->host.pinned_ev) {
    // written by kernels and read by a host that may be polling: fine-grained (coherent) whatever HIP_HOST_COHERENT says
    HIP_TRY(h, hipHostMalloc((void**)&h->host.pinned_ev, sizeof(double) * 16, hipHostMallocCoherent));
    memset(h->host.pinned_ev, 0, sizeof(double) * 16);
  }
  const double* ev = h->host.pinned_ev;
  const double stamp = (double)(++h->host.step);
  launch_step_tail(h->ev.p, h->err_flag.p, h->host.pinned_ev, stamp, st);
  const bool accumulate = h->opt.out_force_accumulate && out_force;
  const size_t rows = h->comm ? (size_t)nlocal : (size_t)ntotal;   // with a communicator the ghost rows have gone home on the device
  if (h->comm) {
    // the pair style's reverse communication, on the device: ghost rows -> their owners' rows (here or on a peer)
    if (ani_comm_reverse(h->comm, h->f64.p, nlocal, st) != ANI_OK) {
      h->err = std::string("ani_comm_reverse: ") + ani_comm_last_error(h->comm);
      return ANI_ERR_DEVICE;
    }
  }
  // Accumulating: the forces come over by a kernel that writes page-locked host memory chunk after chunk and announces every
  // chunk with a word (launch_copy_out); the additions of chunk c run while chunk c + 1 is on its way, and nothing waits for a
  // copy-engine command (each costs ~15 us of gap to its neighbours on this platform).  ANI_FORCE_DMA=1: one copy, then add.
  constexpr int kChunks = HostStaging::kForceChunks;
  const bool polled = accumulate && rows >= 4096 && !getenv("ANI_FORCE_DMA");
  if (accumulate) {
    if (h->host.stage_force_cap < 3 * rows) {
      if (h->host.stage_force) HIP_TRY(h, hipHostFree(h->host.stage_force));
      h->host.stage_force = nullptr;
      h->host.stage_force_cap = 3 * rows + 3 * rows / 2 + 64;
      HIP_TRY(h, hipHostMalloc((void**)&h->host.stage_force, h->host.stage_force_cap * sizeof(double), hipHostMallocCoherent));
    }
    if (polled) {
      if (!h->host.stage_flags) {
        HIP_TRY(h, hipHostMalloc((void**)&h->host.stage_flags, sizeof(unsigned) * kChunks, hipHostMallocCoherent));
        memset(h->host.stage_flags, 0, sizeof(unsigned) * kChunks);
        HIP_TRY(h, h->host.copy_ctr.reserve(kChunks, true));
      }
      h->host.copy_epoch++;
      launch_copy_out(h->f64.p, h->host.stage_force, (long long)(3 * rows), kChunks, h->host.copy_ctr.p, h->host.stage_flags, h->host.copy_epoch,
                      kCopyOutBlocks, st);
    } else {
      HIP_TRY(h, hipMemcpyAsync(h->host.stage_force, h->f64.p, sizeof(double) * 3 * rows, hipMemcpyDeviceToHost, st));
    }
  } else if (out_force) {
    HIP_TRY(h, hipMemcpyAsync(out_force, h->f64.p, sizeof(double) * 3 * rows, hipMemcpyDeviceToHost, st));
    if (rows < (size_t)ntotal) memset(out_force + 3 * rows, 0, sizeof(double) * 3 * ((size_t)ntotal - rows));
  }
  if (eflag_atom && out_atomic_energies)
    HIP_TRY(h, hipMemcpyAsync(out_atomic_energies, h->eatom.p, sizeof(double) * (size_t)nlocal, hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipGetLastError());
  if (polled) {
    // the error word first: nothing may be added on a step that is going to be repeated or reported
    if (!wait_host_word(&h->host.pinned_ev[11], stamp)) { h->err = "the device did not finish the step within 5 s"; return ANI_ERR_DEVICE; }
  } else {
    HIP_TRY(h, hipStreamSynchronize(st));
  }
  const int flag = (int)ev[10];
  if (flag) {
    HIP_TRY(h, hipStreamSynchronize(st));   // a copy-out in flight lands in the staging buffer only
    HIP_TRY(h, hipMemsetAsync(h->err_flag.p, 0, sizeof(int), st));
    h->sticky_flags |= flag;
    if (flag & 2) {
      // a wait between workgroups of the one-launch MLP ran into its bound: a forward-progress problem on the device, not
      // a capacity problem -- no retry with larger lists
      h->err = "a wait inside the one-launch MLP kernel timed out (device-side stall); results of this step are invalid";
      return ANI_ERR_DEVICE;
    }
    h->err = "an atom has more neighbours inside the radial/angular cutoff than the kernels' LDS capacity (radial: the "
             "longest list, or 3/4 of it unless option full_radial_capacity is set; angular: " + std::to_string(kMaxAng) + ")";
    return ANI_ERR_CAPACITY;
  }
  if (accumulate) {
    const double* __restrict__ src = h->host.stage_force;
    double* __restrict__ dst = out_force;
    const long long n = (long long)(3 * rows);
    if (polled) {
      for (int c = 0; c < kChunks; c++) {
        if (!wait_host_word(&h->host.stage_flags[c], h->host.copy_epoch)) { h->err = "the device did not deliver the forces within 5 s"; return ANI_ERR_DEVICE; }
        const long long a = (n * c / kChunks) & ~1LL, b = c + 1 == kChunks ? n : ((n * (c + 1) / kChunks) & ~1LL);   // as copy_out_kernel
        for (long long k = a; k < b; k++) dst[k] += src[k];
      }
      HIP_TRY(h, hipStreamSynchronize(st));   // the kernel has delivered everything: this returns at once (per-atom energies, if any)
    } else {
      for (long long k = 0; k < n; k++) dst[k] += src[k];
    }
  }
  if (out_energy) *out_energy = ev[0];
  if (vflag && out_virial) memcpy(out_virial, ev + 1, sizeof(double) * 9);
  return ANI_OK;
}

// the armed state of a whole-step entry point is cleared on every way out of it
struct ArmedScope { ani_handle* h; ~ArmedScope() { h->armed.av_acc = nullptr; deviation_end(h); } };
}  // namespace ani_host

extern "C" {
int ani_create(const char* model_file, int local_rank, int use_num_models, int use_cuaev, int use_fullnbr, int use_single,
               ani_handle** out) {
  if (out) *out = nullptr;
  if (!model_file || !out) { g_create_error = "null argument"; return ANI_ERR_ARG; }
  if (local_rank < 0) {
    g_create_error = "device 'cpu' (local_rank = -1) is not available: libani_hip is the HIP/gfx950 path only and has no host fallback";
    return ANI_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_error = "no HIP device visible"; return ANI_ERR_DEVICE; }
  ani_handle* h = new ani_handle;
  h->device = local_rank % ndev;  // src/pair_ani.cpp:269-272
  h->use_cuaev = use_cuaev != 0; h->use_fullnbr = use_fullnbr != 0; h->use_single = use_single != 0;
  std::string e = load_model(model_file, use_num_models, h->model);
  if (!e.empty()) { g_create_error = e; delete h; return ANI_ERR_MODEL; }
  if (hipSetDevice(h->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    g_create_error = "cannot initialise HIP device " + std::to_string(h->device);
    delete h;
    return ANI_ERR_DEVICE;
  }
  // the reference's opt-in to reduced-precision products (LAMMPS_ANI_ALLOW_TF32, src/ani_csrc/ani.cpp:41-43): gfx950 has no
  // TF32; the counterpart here is the two-term fp16 split (option "mlp_arith" 2), off unless asked for
  if (const char* tf = getenv("LAMMPS_ANI_ALLOW_TF32")) {
    if (tf[0] && strcmp(tf, "0") != 0) h->opt.mlp_arith = MLP_F16X2;
  }
  if (const char* e = getenv("ANI_AEV_FUSED")) h->opt.aev_fused = atoi(e) != 0;   // experiment knobs: the defaults of the options
  if (const char* e = getenv("ANI_AEV_TICKETS_MIN")) h->opt.aev_tickets_min = atoi(e);
  int rc = upload_model(h);
  if (rc != ANI_OK) { g_create_error = h->err; ani_destroy(h); return rc; }
  // banner, same fields as src/ani_csrc/ani.cpp:88-92
  printf("Successfully loaded the model \nfile: '%s' \ndevice: hip:%d \ndtype: %s \nnbrlist: %s \nani_aev: %s \nuse_num_models: %d/%d\n\n",
         model_file, h->device, h->use_single ? "float (FP32)" : "double (FP64)", h->use_fullnbr ? "full" : "half", h->use_cuaev ? "cuaev" : "pyaev", h->model.M, h->model.M_file);
  fflush(stdout);
  *out = h;
  return ANI_OK;
}

void ani_destroy(ani_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->host.pinned_ints) { (void)hipHostFree(h->host.pinned_ints); h->host.pinned_ints = nullptr; }
  if (h->host.stage_force) { (void)hipHostFree(h->host.stage_force); h->host.stage_force = nullptr; }
  if (h->host.pinned_ev) { (void)hipHostFree(h->host.pinned_ev); h->host.pinned_ev = nullptr; }
  if (h->host.stage_flags) { (void)hipHostFree(h->host.stage_flags); h->host.stage_flags = nullptr; }
  h->host.copy_ctr.release();
  if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
  if (h->ev_mlp) (void)hipEventDestroy(h->ev_mlp);
  if (h->ev_side) (void)hipEventDestroy(h->ev_side);
  for (auto& n : h->nets) {
    for (float* p : n.W) if (p) (void)hipFree(p);
    for (float* p : n.b) if (p) (void)hipFree(p);
    for (float* p : n.WT) if (p) (void)hipFree(p);
    if (n.W0c) (void)hipFree(n.W0c);
    if (n.WT0c) (void)hipFree(n.WT0c);
    if (n.w_out) (void)hipFree(n.w_out);
    if (n.b_out) (void)hipFree(n.b_out);
    for (auto& sp : n.sp) {
      for (unsigned short* p : sp.W) if (p) (void)hipFree(p);
      for (unsigned short* p : sp.WT) if (p) (void)hipFree(p);
      if (sp.W0c) (void)hipFree(sp.W0c);
      if (sp.WT0c) (void)hipFree(sp.WT0c);
    }
    for (double* p : n.W64) if (p) (void)hipFree(p);
    for (double* p : n.b64) if (p) (void)hipFree(p);
    for (double* p : n.WT64) if (p) (void)hipFree(p);
    if (n.W0c64) (void)hipFree(n.W0c64);
    if (n.WT0c64) (void)hipFree(n.WT0c64);
    if (n.w_out64) (void)hipFree(n.w_out64);
    if (n.b_out64) (void)hipFree(n.b_out64);
  }
  h->species.release(); h->ilist.release(); h->numneigh.release(); h->jlist.release(); h->jraw.release(); h->nbr_off.release();
  h->fold_head.release(); h->fold_next.release(); h->fold_bad.release(); h->nb.ovf.release(); h->nb.xq.release(); h->row_of_centre.release(); h->centre_of_row.release(); h->bucket_info.release(); h->err_flag.release(); h->row_ctr.release(); h->row_of_atom.release();
  h->xyzs.release(); h->cl_xyz.release(); h->cl_hdr.release(); h->cl_j.release(); h->row_info.release(); h->row_flag.release(); h->row_list.release(); h->row_count.release(); h->x64.release(); h->f64.release(); h->ev.release(); h->eatom.release(); h->origin.release();
  h->rep_tables.release(); h->erep.release();
  h->nb.cell_id.release(); h->nb.cell_count.release(); h->nb.cell_start.release(); h->nb.cursor.release(); h->nb.order.release(); h->nb.xs.release();
  h->armed.avir.release(); h->armed.avir64.release(); h->armed.avout.release();
  h->armed.gaev_parts64.release(); h->armed.dv_fbuf.release(); h->armed.dv_fbuf64.release(); h->armed.dv_tmp.release(); h->armed.dv_stage.release();
  h->armed.dv_part.release(); h->armed.dv_ticket.release();
  h->mol.bond_cut2.release(); h->mol.ints.release(); h->mol.words.release(); h->mol.owner.release(); h->mol.summary.release(); h->mol.out.release();
  h->rdf.ints.release(); h->rdf.words.release();
  h->virial_acc.release(); h->aev.release(); h->gaev.release(); h->act.release(); h->aev64.release(); h->gaev64.release(); h->act64.release(); h->e_rows64.release(); h->fbuf64.release(); h->e_rows.release(); h->fbuf.release();
  for (int fi = 0; fi < 4; fi++) free_fused(h, fi);
  h->fused.counter.release(); h->fused.gaev_parts.release(); h->fused.sched.release();
  h->stab.desc_b.release(); h->stab.desc_f.release(); h->stab.words_b.release(); h->stab.words_f.release();
  free_chain_plan(h->chain_plan);
  for (auto& e : h->timing.evt_pool) if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

const char* ani_last_error(const ani_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }
int ani_num_models(const ani_handle* h) { return h ? h->model.M_file : 0; }
int ani_use_num_models(const ani_handle* h) { return h ? h->model.M : 0; }
int ani_num_species(const ani_handle* h) { return h ? h->model.S : 0; }
int ani_aev_length(const ani_handle* h) { return h ? h->model.aev_len : 0; }
double ani_cutoff_radial(const ani_handle* h) { return h ? h->model.Rcr : 0; }
double ani_cutoff_angular(const ani_handle* h) { return h ? h->model.Rca : 0; }
const char* ani_species_symbol(const ani_handle* h, int s) {
  return h && s >= 0 && s < h->model.S ? h->model.symbols[s].c_str() : "";
}

int ani_compute_full_device(ani_handle* h, int ntotal, int nlocal, const int* d_species, const double* d_x, int64_t npairs,
                            const int* d_ilist, const int* d_jlist, const int* d_numneigh, int ago, int eflag_atom, int vflag,
                            double* d_f, double* d_ev, double* d_eatom, void* stream) {
  int av_ncomp = 0;
  double* const av_out = take_atom_virial(h, &av_ncomp);
  const DevOut dv = take_deviation(h);
  int rc = check_args(h, ntotal, nlocal, npairs, ago);
  if (rc) return rc;
  if (!d_x || !d_ev) { h->err = "null device pointer"; return ANI_ERR_ARG; }
  {
    // the fold this call runs with: a list of the call (ago == 0) drops the installed one and takes a staged one (rebuild)
    const bool fold = ago == 0 ? (h->stage_nghost >= 0 && h->stage_owner && h->stage_nghost == ntotal - nlocal) : h->fold_nghost >= 0;
    rc = deviation_check(h, dv, ntotal, nlocal, /*device=*/true, fold);
    if (rc) return rc;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default stream (what torch's default stream is)
  if (ago == 0) {
    if (!d_species || !d_ilist || !d_jlist || !d_numneigh) { h->err = "null list pointer with ago == 0"; return ANI_ERR_ARG; }
    // A device-resident caller cannot be handed ANI_ERR_CAPACITY and retried (nothing synchronises; the energy turns NaN
    // and a loop notices steps later): the radial lists get the capacity of the longest candidate list from the start.
    // (The 3/4 estimate of the host entry points saves LDS only; they repeat the step when it was too small.)
    h->ap.full_cap = h->ap_run.full_cap = 1;
    rc = ingest_list(h, ntotal, nlocal, npairs, d_species, d_ilist, d_numneigh, d_jlist, hipMemcpyDeviceToDevice, st);
    if (rc) return rc;
  }
  const ArmedScope armed_scope{h};
  rc = atom_virial_begin(h, av_out != nullptr);
  if (!rc) rc = deviation_begin(h, dv, /*fold=*/true);
  if (rc) return rc;
  rc = run_step(h, d_x, eflag_atom, vflag, d_f, /*accumulate=*/h->opt.dev_overwrite ? 0 : 1, d_ev, d_eatom, st, /*fold=*/true);
  if (rc == ANI_OK && av_out) atom_virial_out(h, av_out, av_ncomp, h->opt.dev_overwrite ? 0 : 1, /*fold=*/true, st);
  // LAMMPS_ANI_PROFILING (src/pair_ani_kokkos.cpp:68-70,210-212): the host's timers see the device work of this call
  if (rc == ANI_OK && h->opt.profiling) HIP_TRY(h, hipStreamSynchronize(st));
  return rc;
}

// ---- split step: see include/ani_hip.h ----------------------------------------------------------------------
static StepCtx split_ctx(const ani_handle* h) {
  StepCtx c;
  c.d_x = h->split.d_x; c.eflag_atom = h->split.eflag_atom; c.vflag = h->split.vflag; c.f_accumulate = h->opt.dev_overwrite ? 0 : 1;
  c.d_f = h->split.d_f; c.d_ev = h->split.d_ev; c.d_eatom = h->split.d_eatom;
  return c;
}

int ani_step_begin(ani_handle* h, int ntotal, int nlocal, const double* d_x, int eflag_atom, int vflag, double* d_f, double* d_ev,
                   double* d_eatom, void* stream) {
  int av_ncomp = 0;
  double* const av_out = take_atom_virial(h, &av_ncomp);
  if (dv_any(take_deviation(h))) {
    h->err = "ani_request_model_deviation: the split step (ani_step_begin) cannot return a model deviation; use a whole-step entry";
    return ANI_ERR_ARG;
  }
  int rc = check_args(h, ntotal, nlocal, 0, /*ago=*/1);
  if (rc) return rc;
  if (!d_x || !d_ev) { h->err = "null device pointer"; return ANI_ERR_ARG; }
  if (h->split_phase != 0) { h->err = "ani_step_begin: the previous split step was not finished"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  h->split.d_x = d_x; h->split.eflag_atom = eflag_atom; h->split.vflag = vflag; h->split.d_f = d_f; h->split.d_ev = d_ev; h->split.d_eatom = d_eatom;
  // an armed split step: both backward halves add to one accumulator, ani_step_finish converts it
  rc = atom_virial_begin(h, av_out != nullptr);
  if (rc) return rc;
  h->armed.split_av = av_out;
  h->armed.split_av_ncomp = av_ncomp;
  h->split_phase = 1;
  if (!split_supported(h)) return ANI_OK;   // the whole step runs in ani_step_ghosts_ready
  rc = ensure_row_classes(h, st);
  if (rc) { h->split_phase = 0; return rc; }
  const StepCtx c = split_ctx(h);
  TraceRange tr("ani: step, rows without ghosts: pack + compaction + AEV forward");
  rc = step_prologue(h, c, false, st);
  if (rc) { h->split_phase = 0; return rc; }
  step_pack(h, c, 0, h->nlocal, true, st);
  if (h->armed.av_acc) HIP_TRY(h, hipMemsetAsync(h->armed.av_acc, 0, sizeof(float) * 9 * (size_t)h->ntotal, st));
  rc = step_compact_forward(h, step_aev_args(h, c, 2), st);
  if (rc) { h->split_phase = 0; return rc; }
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, take_launch_error());
  return ANI_OK;
}

int ani_step_ghosts_ready(ani_handle* h, void* stream) {
  if (!h) return ANI_ERR_ARG;
  if (h->split_phase != 1) { h->err = "ani_step_ghosts_ready without ani_step_begin"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const StepCtx c = split_ctx(h);
  h->split_phase = 2;
  if (!split_supported(h)) {
    const int rc = run_step(h, c.d_x, c.eflag_atom, c.vflag, c.d_f, c.f_accumulate, c.d_ev, c.d_eatom, st);
    if (rc) h->split_phase = 0;
    return rc;
  }
  TraceRange tr("ani: step, rows with ghosts + MLP + their backward pass");
  step_pack(h, c, h->nlocal, h->ntotal, false, st);
  const AevArgs a = step_aev_args(h, c, 1);
  int rc = step_compact_forward(h, a, st);
  if (!rc) rc = compute_mlp(h, st);
  if (rc) { h->split_phase = 0; return rc; }
  if (!h->side) {
    int lo = 0, hi = 0;
    HIP_TRY(h, hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = the numerically largest value = the least urgent
    HIP_TRY(h, hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_mlp, hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_side, hipEventDisableTiming));
  }
  HIP_TRY(h, hipEventRecord(h->ev_mlp, st));
  rc = step_backward(h, c, a, st);
  if (rc) { h->split_phase = 0; return rc; }
  step_finish(h, c, h->nlocal, h->ntotal, false, st);   // the ghost atoms' forces are complete: no other row touches them
  // the other rows' backward pass, beside the above (launched second, on the less urgent stream)
  HIP_TRY(h, hipStreamWaitEvent(h->side, h->ev_mlp, 0));
  rc = step_backward(h, c, step_aev_args(h, c, 2), h->side);
  if (rc) { h->split_phase = 0; return rc; }
  HIP_TRY(h, hipEventRecord(h->ev_side, h->side));
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, take_launch_error());
  return ANI_OK;
}

int ani_step_finish(ani_handle* h, void* stream) {
  if (!h) return ANI_ERR_ARG;
  if (h->split_phase != 2) { h->err = "ani_step_finish without ani_step_ghosts_ready"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  h->split_phase = 0;
  double* const av_out = h->armed.split_av;
  h->armed.split_av = nullptr;
  if (!split_supported(h)) {
    if (av_out) atom_virial_out(h, av_out, h->armed.split_av_ncomp, h->opt.dev_overwrite ? 0 : 1, /*fold=*/false, st);
    h->armed.av_acc = nullptr;
    HIP_TRY(h, hipGetLastError());
    return ANI_OK;
  }
  const StepCtx c = split_ctx(h);
  TraceRange tr("ani: step, finish");
  HIP_TRY(h, hipStreamWaitEvent(st, h->ev_side, 0));   // the backward pass launched by ani_step_ghosts_ready on the side stream
  step_finish(h, c, 0, h->nlocal, true, st);
  if (av_out) atom_virial_out(h, av_out, h->armed.split_av_ncomp, h->opt.dev_overwrite ? 0 : 1, /*fold=*/false, st);
  h->armed.av_acc = nullptr;
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, take_launch_error());
  if (h->opt.profiling) HIP_TRY(h, hipStreamSynchronize(st));
  return ANI_OK;
}

int ani_compute_full(ani_handle* h, int ntotal, int nlocal, const int64_t* species, const double* coordinates, int64_t npairs,
                     const int* ilist_unique, const int* jlist, const int* numneigh, int ago, int eflag_atom, int vflag,
                     double* out_energy, double* out_force, double* out_atomic_energies, double* out_virial) {
  int av_ncomp = 0;
  double* const av_out = take_atom_virial(h, &av_ncomp);
  const DevOut dv = take_deviation(h);
  int rc = check_args(h, ntotal, nlocal, npairs, ago);
  if (rc) return rc;
  if (!coordinates || !out_force || !out_energy) { h->err = "null pointer argument"; return ANI_ERR_ARG; }
  rc = deviation_check(h, dv, ntotal, nlocal, /*device=*/false, /*fold=*/false);
  if (rc) return rc;
  if (av_out && h->comm) {
    // the ghost rows would have to go home through a 9-wide reverse exchange, which ani_comm does not have
    h->err = "ani_request_atom_virial: the host entry points cannot return a per-atom virial with a communicator attached "
             "(ani_attach_comm); detach it and reverse-communicate the ghost rows, or use ani_compute_full_device";
    return ANI_ERR_ARG;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  if (h->comm && h->use_cuaev && !(h->ap.full_cap && h->ap_run.full_cap)) {
    // With a communicator attached the step ends in a matched send / receive with every peer (finish_host), posted before
    // the capacity word is read.  The retry below would post a SECOND exchange on this rank alone: its peers have added the
    // overflowed step's ghost forces already and pair the extra message with their next step (forces one step stale, or a
    // hang at destroy).  So no retry can happen here: the lists are sized for the worst case from the start, as for the
    // device entry points.
    h->ap.full_cap = h->ap_run.full_cap = 1;
    if (ago != 0) {
      rc = rebuild(h, st);
      if (rc) return rc;
    }
  }
  if (ago == 0) {
    if (!species || !ilist_unique || !numneigh || (npairs > 0 && !jlist)) { h->err = "null list pointer with ago == 0"; return ANI_ERR_ARG; }
    h->host.species32.resize(ntotal);
    for (int i = 0; i < ntotal; i++) h->host.species32[i] = (int)species[i];
    rc = ingest_list(h, ntotal, nlocal, npairs, h->host.species32.data(), ilist_unique, numneigh, jlist, hipMemcpyHostToDevice, st);
    if (rc) return rc;
  }
  HIP_TRY(h, h->x64.reserve((size_t)ntotal * 3));
  HIP_TRY(h, h->f64.reserve((size_t)ntotal * 3));
  HIP_TRY(h, h->ev.reserve(10));
  HIP_TRY(h, h->eatom.reserve(std::max(nlocal, 1)));
  if (h->host.x64_from != coordinates)   // (a re-neighbouring step of the `devlist` mode: ani_build_list uploaded them a moment ago)
    HIP_TRY(h, hipMemcpyAsync(h->x64.p, coordinates, sizeof(double) * 3 * (size_t)ntotal, hipMemcpyHostToDevice, st));
  h->host.x64_from = nullptr;
  if (av_out) HIP_TRY(h, h->armed.avout.reserve((size_t)std::max(ntotal, 1) * av_ncomp));
  const ArmedScope armed_scope{h};
  DevStage dvs;
  rc = atom_virial_begin(h, av_out != nullptr);
  if (!rc) rc = deviation_stage(h, dv, ntotal, nlocal, &dvs);
  if (!rc) rc = deviation_begin(h, dvs.dev, /*fold=*/false);
  if (rc) return rc;
  // the step, then what was armed (every ntotal row of the per-atom virial, ghosts included: the caller folds them like the forces)
  auto step_and_finish = [&]() -> int {
    int r = run_step(h, h->x64.p, eflag_atom, vflag, h->f64.p, /*accumulate=*/0, h->ev.p, h->eatom.p, st);
    if (!r && av_out) {
      atom_virial_out(h, h->armed.avout.p, av_ncomp, /*accumulate=*/0, /*fold=*/false, st);
      HIP_TRY(h, hipMemcpyAsync(av_out, h->armed.avout.p, sizeof(double) * av_ncomp * (size_t)ntotal, hipMemcpyDeviceToHost, st));
    }
    if (!r && h->armed.dv_on) r = deviation_copy_home(h, dv, dvs, st);
    return r ? r : finish_host(h, ntotal, nlocal, eflag_atom, vflag, out_energy, out_force, out_atomic_energies, out_virial);
  };
  rc = step_and_finish();
  if (rc == ANI_ERR_CAPACITY && h->use_cuaev && !h->ap_run.full_cap && !h->comm) {
    // The screened radial lists are sized for 3/4 of the longest candidate list; a system denser than that inside Rcr
    // (small skin, compressed fluid) is input the reference handles, so the step is repeated once with the capacity of
    // the full list and the setting kept for the rest of the run.  An overflow that survives (more than kMaxAng
    // neighbours inside Rca) is still reported.
    h->ap.full_cap = h->ap_run.full_cap = 1;
    fprintf(stderr, "libani_hip: radial neighbour capacity exceeded, continuing with full_radial_capacity = 1\n");
    rc = rebuild(h, st);
    if (!rc) rc = step_and_finish();
  }
  if (rc == ANI_OK && (av_out || h->armed.dv_on)) HIP_TRY(h, hipStreamSynchronize(st));
  return rc;
}

int ani_compute_half(ani_handle* h, int ntotal, int nlocal, const int64_t* species, const double* coordinates, int64_t npairs_half,
                     const int64_t* atom_index12, int ago, int eflag_atom, int vflag, double* out_energy, double* out_force,
                     double* out_atomic_energies, double* out_virial) {
  if (!h) return ANI_ERR_ARG;
  // A half pair feeds both of its local ends (src/ani_csrc/ani.cpp:100-180: every atom < nlocal is a centre), so the
  // half list is expanded once per rebuild into the per-centre form the kernels consume.
  if (ago == 0) {
    // an armed call that fails still takes the arming
    auto refuse = [h](const char* why) { h->err = why; h->armed.av_out = nullptr; h->armed.dv_req = DevOut{}; return ANI_ERR_ARG; };
    if (!atom_index12 && npairs_half > 0) return refuse("null atom_index12 with ago == 0");
    std::vector<int>& num = h->host.half_num;
    std::vector<int>& jl = h->host.half_j;
    num.assign(nlocal, 0);
    for (int64_t p = 0; p < npairs_half; p++) {
      const int64_t a = atom_index12[p], b = atom_index12[npairs_half + p];
      if (a < 0 || a >= ntotal || b < 0 || b >= ntotal) return refuse("atom_index12 entry out of range");
      if (a < nlocal) num[a]++;
      if (b < nlocal) num[b]++;
    }
    std::vector<int64_t> off(nlocal + 1, 0);
    for (int i = 0; i < nlocal; i++) off[i + 1] = off[i] + num[i];
    jl.resize(off[nlocal]);
    std::vector<int64_t> fill(off.begin(), off.end() - 1);
    for (int64_t p = 0; p < npairs_half; p++) {
      const int64_t a = atom_index12[p], b = atom_index12[npairs_half + p];
      if (a < nlocal) jl[fill[a]++] = (int)b;
      if (b < nlocal) jl[fill[b]++] = (int)a;
    }
    std::vector<int> il(nlocal);
    for (int i = 0; i < nlocal; i++) il[i] = i;
    return ani_compute_full(h, ntotal, nlocal, species, coordinates, (int64_t)jl.size(), il.data(), jl.data(), num.data(), 0,
                            eflag_atom, vflag, out_energy, out_force, out_atomic_energies, out_virial);
  }
  return ani_compute_full(h, ntotal, nlocal, species, coordinates, h->npairs, nullptr, nullptr, nullptr, ago, eflag_atom, vflag,
                          out_energy, out_force, out_atomic_energies, out_virial);
}

// Page-locking of caller arrays for the host entry points: explicit, because a registration belongs to an address range and
// only the owner of the memory knows when that range stops meaning the same pages.
int ani_host_register(const void* p, size_t bytes) {
  if (!p || bytes == 0) return ANI_ERR_ARG;
  if (hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return ANI_ERR_DEVICE; }
  return ANI_OK;
}
int ani_host_unregister(const void* p) {
  if (!p) return ANI_ERR_ARG;
  if (hipHostUnregister(const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return ANI_ERR_DEVICE; }
  return ANI_OK;
}

int ani_attach_comm(ani_handle* h, void* comm) {
  if (!h) return ANI_ERR_ARG;
  h->comm = static_cast<ani_comm*>(comm);
  return ANI_OK;
}
}  // extern "C"
