// ani_hip_list.cpp — the list of an epoch: ingest, device-side build, rebuild(), ghost folds, row classes.  Internal: see ani_handle.h.
#include "ani_handle.h"

namespace ani_host __attribute__((visibility("hidden"))) {
constexpr int kRebuildRowsOverflow = -1000;   // internal: the rows of launch_nbr_sorted_rows were too short
// (re)build everything that depends on the neighbour list: offsets, species buckets, activation arena.
// d_species/d_ilist/d_numneigh/d_jlist already hold this epoch's list in the handle's own buffers.
int rebuild(ani_handle* h, hipStream_t st) {
  const HostModel& m = h->model;
  roctxMarkA("neighbor list rebuilt");   // src/ani_csrc/ani.cpp:128,215
  TraceRange tr("ani: list epoch set-up (offsets, species buckets, segment sort)");
  h->need_origin = !h->origin_from_box;
  h->fold_nghost = -1;       // the maps belonged to the list before
  h->classes_valid = false;
  h->split_phase = 0;
  const int nlocal = h->nlocal;
  const int nrows_cap = round_up(nlocal, kRowTile) + m.S * kRowTile;
  HIP_TRY(h, h->nbr_off.reserve((size_t)nlocal + 1));
  HIP_TRY(h, h->row_of_centre.reserve(prepare_scratch_ints(nlocal)));
  HIP_TRY(h, h->centre_of_row.reserve(nrows_cap));
  HIP_TRY(h, h->row_info.reserve(nrows_cap));
  HIP_TRY(h, h->bucket_info.reserve(kBucketInfoInts));
  // a capacity overflow of an earlier epoch must not poison this one (the flag turns the device path's energy into NaN)
  HIP_TRY(h, h->err_flag.reserve(1, true));
  // ... but what it said is kept: the device path only turns the energy into NaN, and a caller that looks at the energy
  // every few steps must still be able to tell a capacity overflow from a stalled kernel (ani_debug_get: error_flags).  The
  // word travels to a page-locked host word without a synchronisation of its own: it is read behind the one the bucket
  // counts below need anyway.
  if (!h->host.pinned_ints) HIP_TRY(h, hipHostMalloc((void**)&h->host.pinned_ints, sizeof(int) * 32, hipHostMallocDefault));
  h->host.pinned_ints[0] = h->host.pinned_ints[1] = h->host.pinned_ints[2] = 0;
  HIP_TRY(h, hipMemcpyAsync(&h->host.pinned_ints[0], h->err_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipMemsetAsync(h->err_flag.p, 0, sizeof(int), st));
  HIP_TRY(h, h->row_of_atom.reserve((size_t)std::max(h->ntotal, 1)));
  PrepOut o{h->nbr_off.p, h->row_of_centre.p, h->centre_of_row.p, h->row_info.p, h->bucket_info.p, h->row_of_atom.p};
  launch_prepare(h->species.p, h->ilist.p, h->numneigh.p, nlocal, h->ntotal, m.S, nrows_cap, o, st, h->jlist_row_stride);
  if (h->jlist_row_stride) HIP_TRY(h, hipMemcpyAsync(&h->host.pinned_ints[1], h->nb.ovf.p, sizeof(int), hipMemcpyDeviceToHost, st));
  // a staged ghost fold: its chains are made here, its check rides on the synchronisation below
  const bool fold_staged = h->stage_nghost >= 0 && h->stage_owner && h->use_single && h->stage_nghost == h->ntotal - nlocal;
  if (fold_staged) {
    HIP_TRY(h, h->fold_head.reserve((size_t)std::max(nlocal, 1)));
    HIP_TRY(h, h->fold_next.reserve((size_t)std::max(h->stage_nghost, 1)));
    HIP_TRY(h, h->fold_bad.reserve(1));
    launch_ghost_chain(reinterpret_cast<const long long*>(h->stage_owner), h->stage_nghost, nlocal, h->fold_head.p, h->fold_next.p, h->fold_bad.p, st);
    HIP_TRY(h, hipMemcpyAsync(&h->host.pinned_ints[2], h->fold_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  int info[kBucketInfoInts];
  HIP_TRY(h, hipMemcpyAsync(info, h->bucket_info.p, sizeof(info), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));
  h->sticky_flags |= h->host.pinned_ints[0];   // the error word of the epoch before (copied above)
  HIP_TRY(h, take_launch_error());
  if (h->jlist_row_stride && h->host.pinned_ints[1]) return kRebuildRowsOverflow;   // build_list fills dense segments instead
  if (h->jlist_row_stride) h->npairs = info[2 * kMaxSpecies + 4];
  if (fold_staged) {
    if (h->host.pinned_ints[2]) { h->stage_nghost = -1; h->err = "ani_stage_ghost_fold: an owner index lies outside [0, nlocal)"; return ANI_ERR_ARG; }
    h->fold.owner = reinterpret_cast<const long long*>(h->stage_owner); h->fold.shift = h->stage_shift; h->fold.nlocal = nlocal;
    h->fold_nghost = h->stage_nghost;
  }
  h->stage_nghost = -1;
  if (info[2 * kMaxSpecies + 1]) { h->err = "an atom has a species outside the model's species list (or ilist holds an index outside [0, ntotal))"; return ANI_ERR_ARG; }
  for (int s = 0; s < m.S; s++) { h->count[s] = info[s]; h->row_start[s] = info[kMaxSpecies + s]; }
  h->nrows = info[2 * kMaxSpecies];
  h->max_numneigh = info[2 * kMaxSpecies + 2];
  {
    const int rcs = specialize(h, info[2 * kMaxSpecies + 3]);
    if (rcs) return rcs;
    const int rct = build_stream_tables(h, st);   // once per species map, not per list
    if (rct) return rct;
  }
  // A caller's list is checked for symmetry once per epoch (the symmetric radial collection relies on it); one that fails
  // runs with the scatter of every term, which is right for any list.  Said once.
  h->list_symmetric = true;
  if (!h->list_is_ours && h->use_single && h->opt.aev_sym_radial && nlocal > 0) {
    HIP_TRY(h, h->sym_acc.reserve((size_t)std::max(h->ntotal, 1)));
    launch_list_symmetry(h->ilist.p, h->nbr_off.p, h->numneigh.p, h->jraw.p, h->row_of_atom.p, nlocal, h->ntotal, h->sym_acc.p,
                         h->bucket_info.p, st);   // bucket_info has been read: its first word carries the verdict
    int bad = 0;
    HIP_TRY(h, hipMemcpyAsync(&bad, h->bucket_info.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    HIP_TRY(h, take_launch_error());
    if (bad) {
      h->list_symmetric = false;
      h->sticky_flags |= 8;
      if (!h->warned_asymmetric) {
        h->warned_asymmetric = true;
        fprintf(stderr, "libani_hip: the neighbour list is not symmetric between owned atoms (j in i's list without i in j's): "
                        "aev_symmetric_radial is off for such epochs, every radial term is scattered\n");
      }
    }
  }
  // neighbour segments grouped by species: what lets the AEV kernels accumulate without atomics (launch_nbr_sorted_rows
  // leaves its rows that way)
  if (!h->jlist_row_stride) launch_sort_jlist(h->species.p, h->nbr_off.p, h->numneigh.p, h->jraw.p, h->jlist.p, nlocal, m.S, info[2 * kMaxSpecies + 3], st, h->jraw_stride);

  const size_t stride = h->ap_run.aev_stride;
  if (!h->use_single) {
    HIP_TRY(h, h->aev64.reserve((size_t)std::max(h->nrows, 1) * stride));
    HIP_TRY(h, h->gaev64.reserve((size_t)std::max(h->nrows, 1) * stride));
    HIP_TRY(h, hipMemsetAsync(h->aev64.p, 0, (size_t)h->nrows * stride * sizeof(double), st));
    HIP_TRY(h, h->e_rows64.reserve((size_t)m.M * std::max(h->nrows, 1)));
    size_t need64 = 0;
    for (int s = 0; s < m.S; s++)
      for (int k = 1; k < m.L; k++) need64 += (size_t)round_up(h->count[s], kRowTile) * m.M * h->nets[s].w[k];
    HIP_TRY(h, h->act64.reserve(std::max<size_t>(need64, 1)));
    HIP_TRY(h, hipMemsetAsync(h->act64.p, 0, need64 * sizeof(double), st));
    h->Hbuf64.assign(m.S, std::vector<double*>(m.L, nullptr));
    size_t off64 = 0;
    for (int s = 0; s < m.S; s++)
      for (int k = 1; k < m.L; k++) {
        h->Hbuf64[s][k] = h->act64.p + off64;
        off64 += (size_t)round_up(h->count[s], kRowTile) * m.M * h->nets[s].w[k];
      }
    return ANI_OK;
  }
  HIP_TRY(h, h->aev.reserve((size_t)std::max(h->nrows, 1) * stride));
  HIP_TRY(h, h->gaev.reserve((size_t)std::max(h->nrows, 1) * stride));
  HIP_TRY(h, hipMemsetAsync(h->aev.p, 0, (size_t)h->nrows * stride * sizeof(float), st));  // padding rows stay zero
  HIP_TRY(h, h->e_rows.reserve((size_t)m.M * std::max(h->nrows, 1)));
  // per-step compact neighbour lists of the fast AEV path
  h->cl_stride = aev_compact_stride(h->ap_run, h->max_numneigh);
  if (h->cl_stride > 0) {
    HIP_TRY(h, h->cl_hdr.reserve((size_t)2 * std::max(h->nrows, 1)));
    HIP_TRY(h, h->cl_xyz.reserve((size_t)std::max(h->nrows, 1) * h->cl_stride));
    HIP_TRY(h, h->cl_j.reserve((size_t)std::max(h->nrows, 1) * h->cl_stride));
  }

  h->arena_valid = false;   // the per-layer kernels' activation arena is laid out when they first run in this epoch
  return ANI_OK;
}

// The list a whole-step entry point is handed at ago == 0 -> the handle's buffers, then the epoch set-up.  kind: where the four
// arrays live (the device entry's on the device, the host entry's on the host, its species already narrowed to int).
int ingest_list(ani_handle* h, int ntotal, int nlocal, long long npairs, const int* species, const int* ilist, const int* numneigh,
                const int* jlist, hipMemcpyKind kind, hipStream_t st) {
  h->ntotal = ntotal; h->nlocal = nlocal; h->npairs = npairs;
  HIP_TRY(h, h->species.reserve(ntotal));
  HIP_TRY(h, h->ilist.reserve(nlocal));
  HIP_TRY(h, h->numneigh.reserve(nlocal));
  HIP_TRY(h, h->jlist.reserve(npairs));
  HIP_TRY(h, h->jraw.reserve(npairs));
  HIP_TRY(h, hipMemcpyAsync(h->species.p, species, sizeof(int) * (size_t)ntotal, kind, st));
  HIP_TRY(h, hipMemcpyAsync(h->ilist.p, ilist, sizeof(int) * (size_t)nlocal, kind, st));
  HIP_TRY(h, hipMemcpyAsync(h->numneigh.p, numneigh, sizeof(int) * (size_t)nlocal, kind, st));
  HIP_TRY(h, hipMemcpyAsync(h->jraw.p, jlist, sizeof(int) * (size_t)npairs, kind, st));
  h->have_list = false;
  h->list_is_ours = false;
  h->jraw_stride = h->jlist_row_stride = 0;
  h->origin_from_box = false;
  const int rc = rebuild(h, st);
  if (rc) return rc;
  h->have_list = true;
  return ANI_OK;
}

// Split step (include/ani_hip.h, ani_step_*).  The rows are classed once per list epoch, on first use.
int ensure_row_classes(ani_handle* h, hipStream_t st) {
  if (h->classes_valid) return ANI_OK;
  HIP_TRY(h, h->row_flag.reserve(std::max(h->nrows, 1)));
  HIP_TRY(h, h->row_list.reserve(std::max(h->nrows, 1)));
  HIP_TRY(h, h->row_count.reserve(1));
  launch_row_classes(h->row_info.p, h->jlist.p, h->nrows, h->nlocal, h->row_flag.p, h->row_list.p, h->row_count.p, st);
  int nb = 0;
  HIP_TRY(h, hipMemcpyAsync(&nb, h->row_count.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));   // once per re-neighbouring
  h->n_boundary = nb;
  h->classes_valid = true;
  return ANI_OK;
}

// the list build proper; d_species may be h->species.p itself (already in place) or a caller's device array
int build_list(ani_handle* h, int ntotal, int nlocal, const int* d_species, const double* d_x, double cutneigh, const double* lo,
               const double* hi, int64_t* out_npairs, hipStream_t st) {
  int rc = 0;
  NbrGrid g;
  long long ncell = 1;
  for (int k = 0; k < 3; k++) {
    const double len = hi[k] - lo[k];
    if (!(len > 0)) { h->err = "empty bounding box"; return ANI_ERR_ARG; }
    int nc = (int)(len / (h->opt.nbr_half_cells ? 0.5 * cutneigh : cutneigh));
    nc = std::max(1, std::min(nc, 1024));
    g.lo[k] = lo[k]; g.inv[k] = nc / len; g.nc[k] = nc;
    ncell *= nc;
  }
  if (ncell > (1LL << 26)) { h->err = "bounding box too large for the cell grid"; return ANI_ERR_ARG; }
  g.ncell = (int)ncell;
  g.reach = h->opt.nbr_half_cells ? 2 : 1;
  h->have_list = false;
  h->ntotal = ntotal; h->nlocal = nlocal;
  HIP_TRY(h, h->nb.cell_id.reserve(ntotal));
  HIP_TRY(h, h->nb.cell_count.reserve((size_t)g.ncell + 1));
  HIP_TRY(h, h->nb.cell_start.reserve((size_t)g.ncell + 1));
  HIP_TRY(h, h->nb.cursor.reserve(g.ncell));
  HIP_TRY(h, h->nb.order.reserve(ntotal));
  HIP_TRY(h, h->nb.xs.reserve((size_t)3 * ntotal));
  HIP_TRY(h, h->species.reserve(ntotal));
  HIP_TRY(h, h->ilist.reserve(nlocal));
  HIP_TRY(h, h->numneigh.reserve(nlocal));
  HIP_TRY(h, h->nbr_off.reserve((size_t)nlocal + 1));
  NbrScratch s{h->nb.cell_id.p, h->nb.cell_count.p, h->nb.cell_start.p, h->nb.cursor.p, h->nb.order.p, h->nb.xs.p};
  if (d_species != h->species.p)
    HIP_TRY(h, hipMemcpyAsync(h->species.p, d_species, sizeof(int) * (size_t)ntotal, hipMemcpyDeviceToDevice, st));
  // the epoch's origin (the fp32 positions of the steps are relative to it): the middle of the caller's box, no kernel
  if (!h->host.pinned_ints) HIP_TRY(h, hipHostMalloc((void**)&h->host.pinned_ints, sizeof(int) * 32, hipHostMallocDefault));
  {
    HIP_TRY(h, h->origin.reserve(3));
    double* mid = reinterpret_cast<double*>(h->host.pinned_ints + 8);
    for (int k = 0; k < 3; k++) mid[k] = 0.5 * (lo[k] + hi[k]);
    HIP_TRY(h, hipMemcpyAsync(h->origin.p, mid, 3 * sizeof(double), hipMemcpyHostToDevice, st));
    h->origin_from_box = true;
  }
  h->list_is_ours = true;
  h->jraw_stride = h->jlist_row_stride = 0;
  // Rows of a fixed capacity where the longest list of the build before says how long a row can get; the first build of a
  // handle, and any build that overflows its rows, counts first and fills dense segments (count and fill walk the same cells
  // with the same distance tests: 0.125 + 0.154 ms at 100 002 atoms).
  const int cap = h->nb.cap_hint > 0 ? round_up(h->nb.cap_hint + h->nb.cap_hint / 8 + 8, 8) : 0;
  const bool rows_fit = h->opt.nbr_onepass && cap > 0 && (long long)nlocal * cap < (1LL << 31);
  const bool sorted_rows = rows_fit && h->opt.nbr_sorted_rows && nbr_sorted_rows_supported(ntotal, h->model.S, cap);
  if (sorted_rows) {
    // search and species grouping in one kernel straight into jlist; pair count, overflow word, bucket counts and the check of
    // a staged ghost fold all come back behind the ONE synchronisation of rebuild()
    HIP_TRY(h, h->nb.xq.reserve((size_t)std::max(ntotal, 1)));
    s.xq = h->nb.xq.p;
    launch_nbr_bin(d_x, ntotal, g, s, st, h->species.p);
    HIP_TRY(h, h->nb.ovf.reserve(1));
    HIP_TRY(h, h->jlist.reserve((size_t)std::max(nlocal, 1) * cap));
    launch_nbr_sorted_rows(nlocal, ntotal, g, s, cutneigh, h->model.S, cap, h->numneigh.p, h->ilist.p, h->jlist.p, h->nb.ovf.p, st);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, take_launch_error());
    h->jlist_row_stride = cap;
    rc = rebuild(h, st);
    if (rc != kRebuildRowsOverflow) {
      if (rc) return rc;
      h->nb.cap_hint = h->max_numneigh;
      h->have_list = true;
      if (out_npairs) *out_npairs = h->npairs;
      return ANI_OK;
    }
    h->jlist_row_stride = 0;   // a row was too short: the bins stand, count and fill as below
  } else {
    launch_nbr_bin(d_x, ntotal, g, s, st);
  }
  int total = 0, ovf = 0;
  const bool onepass = rows_fit && !sorted_rows;
  if (onepass) {
    HIP_TRY(h, h->nb.ovf.reserve(1));
    HIP_TRY(h, h->jraw.reserve((size_t)std::max(nlocal, 1) * cap));
    launch_nbr_onepass(nlocal, ntotal, g, s, cutneigh, cap, h->numneigh.p, h->nbr_off.p, h->jraw.p, h->ilist.p, h->nb.ovf.p, st);
    HIP_TRY(h, hipMemcpyAsync(&ovf, h->nb.ovf.p, sizeof(int), hipMemcpyDeviceToHost, st));
  } else {
    launch_nbr_count(nlocal, ntotal, g, s, cutneigh, h->numneigh.p, h->nbr_off.p, st);
  }
  HIP_TRY(h, hipMemcpyAsync(&total, h->nbr_off.p + nlocal, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));  // the pair count sizes the list buffers (rebuild steps only)
  if (total < 0) { h->err = "more than 2^31 neighbour pairs per rank is not supported"; return ANI_ERR_ARG; }
  h->npairs = total;
  HIP_TRY(h, h->jlist.reserve(total));
  if (onepass && !ovf) {
    h->jraw_stride = cap;
  } else {
    HIP_TRY(h, h->jraw.reserve(total));
    launch_nbr_fill(nlocal, ntotal, g, s, cutneigh, h->nbr_off.p, h->jraw.p, h->ilist.p, st);
  }
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, take_launch_error());
  rc = rebuild(h, st);
  if (rc) return rc;
  h->nb.cap_hint = h->max_numneigh;
  h->have_list = true;
  if (out_npairs) *out_npairs = total;
  return ANI_OK;
}

int build_list_args(ani_handle* h, int ntotal, int nlocal, const void* species, const void* x, double cutneigh, const double* lo,
                    const double* hi, const char* who) {
  int rc = check_args(h, ntotal, nlocal, 0, 0);
  if (rc) return rc;
  if (!species || !x || !lo || !hi) { h->err = "null pointer"; return ANI_ERR_ARG; }
  if (!(cutneigh >= h->model.Rcr)) { h->err = "cutneigh must be at least the model's radial cutoff"; return ANI_ERR_ARG; }
  if (!h->use_fullnbr) { h->err = std::string(who) + " builds a full list; the handle was created for half lists"; return ANI_ERR_ARG; }
  return ANI_OK;
}
}  // namespace ani_host

extern "C" {
int ani_build_list_device(ani_handle* h, int ntotal, int nlocal, const int* d_species, const double* d_x, double cutneigh,
                          const double* lo, const double* hi, int64_t* out_npairs, void* stream) {
  const int rc = build_list_args(h, ntotal, nlocal, d_species, d_x, cutneigh, lo, hi, "ani_build_list_device");
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  h->ap.full_cap = h->ap_run.full_cap = 1;   // device-resident callers: see ani_compute_full_device
  return build_list(h, ntotal, nlocal, d_species, d_x, cutneigh, lo, hi, out_npairs, (hipStream_t)stream);
}

int ani_build_list(ani_handle* h, int ntotal, int nlocal, const int64_t* species, const double* coordinates, double cutneigh,
                   const double* lo, const double* hi, int64_t* out_npairs) {
  const int rc = build_list_args(h, ntotal, nlocal, species, coordinates, cutneigh, lo, hi, "ani_build_list");
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  h->host.species32.resize(ntotal);
  for (int i = 0; i < ntotal; i++) h->host.species32[i] = (int)species[i];
  HIP_TRY(h, h->species.reserve(ntotal));
  HIP_TRY(h, h->x64.reserve((size_t)ntotal * 3));
  HIP_TRY(h, hipMemcpyAsync(h->species.p, h->host.species32.data(), sizeof(int) * (size_t)ntotal, hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(h->x64.p, coordinates, sizeof(double) * 3 * (size_t)ntotal, hipMemcpyHostToDevice, st));
  const int rcb = build_list(h, ntotal, nlocal, h->species.p, h->x64.p, cutneigh, lo, hi, out_npairs, st);
  // the step that follows in the same timestep passes the same array with the same contents (include/ani_hip.h): no second upload
  h->host.x64_from = (rcb == ANI_OK && h->opt.reuse_upload) ? coordinates : nullptr;
  return rcb;
}

int ani_set_ghost_fold(ani_handle* h, const int64_t* d_owner, const double* d_shift, int nghost, void* stream) {
  if (!h) return ANI_ERR_ARG;
  if (!d_owner || nghost < 0) { h->fold_nghost = -1; return ANI_OK; }   // cleared
  if (!h->use_single) { h->err = "ani_set_ghost_fold: the fp64 kernels do not fold ghosts (use the exchange kernels)"; return ANI_ERR_ARG; }
  if (!h->have_list || nghost != h->ntotal - h->nlocal) { h->err = "ani_set_ghost_fold: no list installed, or nghost differs from the list's"; return ANI_ERR_ARG; }
  if (!d_shift && nghost > 0) { h->err = "ani_set_ghost_fold: null shift"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(h, h->fold_head.reserve((size_t)std::max(h->nlocal, 1)));
  HIP_TRY(h, h->fold_next.reserve((size_t)std::max(nghost, 1)));
  HIP_TRY(h, h->fold_bad.reserve(1));
  static_assert(sizeof(long long) == sizeof(int64_t), "owner indices are 64-bit");
  launch_ghost_chain(reinterpret_cast<const long long*>(d_owner), nghost, h->nlocal, h->fold_head.p, h->fold_next.p, h->fold_bad.p, st);
  int bad = 0;
  HIP_TRY(h, hipMemcpyAsync(&bad, h->fold_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));   // once per re-neighbouring
  HIP_TRY(h, take_launch_error());
  if (bad) { h->fold_nghost = -1; h->err = "ani_set_ghost_fold: an owner index lies outside [0, nlocal)"; return ANI_ERR_ARG; }
  h->fold.owner = reinterpret_cast<const long long*>(d_owner); h->fold.shift = d_shift; h->fold.nlocal = h->nlocal;
  h->fold_nghost = nghost;
  return ANI_OK;
}

int ani_stage_ghost_fold(ani_handle* h, const int64_t* d_owner, const double* d_shift, int nghost) {
  if (!h) return ANI_ERR_ARG;
  h->stage_owner = nullptr; h->stage_shift = nullptr; h->stage_nghost = -1;
  if (!d_owner || nghost < 0) return ANI_OK;   // cleared
  if (!h->use_single) { h->err = "ani_stage_ghost_fold: the fp64 kernels do not fold ghosts (use the exchange kernels)"; return ANI_ERR_ARG; }
  if (!d_shift && nghost > 0) { h->err = "ani_stage_ghost_fold: null shift"; return ANI_ERR_ARG; }
  h->stage_owner = d_owner; h->stage_shift = d_shift; h->stage_nghost = nghost;
  return ANI_OK;
}
}  // extern "C"
