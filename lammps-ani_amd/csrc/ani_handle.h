// ani_handle.h -- internal to the host side of libani_hip.so (the ani_hip*.cpp files; not a header under include/): the handle
// behind the C ABI, its small helpers and the functions that cross those files.  Everything here but struct ani_handle
// itself lives in a namespace of hidden visibility: nothing of it enters the library's dynamic symbol table.
#pragma once
#include "../../include/ani_hip.h"
#include "../../include/ani_comm.h"

#include <hip/hip_runtime.h>
#ifndef ANI_NO_ROCTX
#include <rocprofiler-sdk-roctx/roctx.h>
#else   // built without the profiler SDK: the markers (only profiling runs look at them) become no-ops
static inline void roctxRangePushA(const char*) {}
static inline void roctxRangePop() {}
static inline void roctxMarkA(const char*) {}
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ani_kernels.h"
#include "ani_model.h"

namespace ani_host __attribute__((visibility("hidden"))) {
using namespace ani;

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  // grow-only, 1.5x policy like the reference's jlist (src/pair_ani.cpp:119-127); contents are NOT preserved
  hipError_t reserve(size_t n, bool zero = false) {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    size_t want = std::max<size_t>(n + n / 2, 64);
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e != hipSuccess) { cap = 0; return e; }
    cap = want;
    // hipMemset on device memory runs on the null stream and may return before it has run; the handle's work is on
    // non-blocking streams, which do not wait for the null stream: wait here (allocation time only)
    if (zero) {
      e = hipMemset(p, 0, want * sizeof(T));
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// roctx range for the profiler's timeline (the reference marks its phases with NVTX: src/pair_ani.cpp:198-200,
// src/ani_csrc/ani.cpp:128,215); costs nothing measurable when no tool is attached
struct TraceRange {
  explicit TraceRange(const char* name) { roctxRangePushA(name); }
  ~TraceRange() { roctxRangePop(); }
  TraceRange(const TraceRange&) = delete;
  TraceRange& operator=(const TraceRange&) = delete;
};

struct SpeciesNet {
  // device weights; layouts described in compute_mlp()
  std::vector<float*> W;    // [L-1]   W[k]: [M][d[k+1]][kpad(k)]        forward, k = 0..L-2
  std::vector<float*> b;    // [L-1]   b[k]: [M][d[k+1]]
  std::vector<float*> WT;   // [L-1]   WT[k], k = 1..L-2: [M][d[k]][w(k+1)] ; WT[0]: [aev_len][M*w(1)]
  float* W0c = nullptr;     // first layer restricted to the AEV columns of the species present: [M][d[1]][aev_stride']
  float* WT0c = nullptr;    // and its transposed copy [aev_len'][M*w(1)]   (null when every species is present)
  float* w_out = nullptr;   // [M][w(L-1)]
  float* b_out = nullptr;   // [M]
  std::vector<int> w;       // w[k] = round_up(d[k],4), k = 0..L-1 (w[0] = aev_stride)
  // double-precision mirrors of the above (precision 'double' only)
  std::vector<double*> W64, b64, WT64;
  double *W0c64 = nullptr, *WT0c64 = nullptr, *w_out64 = nullptr, *b_out64 = nullptr;
  // 16-bit planes of W / WT / W0c / WT0c for the split MFMA paths (blocked [ceil(K/16)][N][planes][16]):
  // sp[0] three bf16 planes (MLP_BF16X3), sp[1] two fp16 planes of wscale[k] * W (MLP_F16X2)
  struct Planes {
    std::vector<unsigned short*> W, WT;
    unsigned short *W0c = nullptr, *WT0c = nullptr;
  } sp[2];
  std::vector<float> wscale;   // [L-1] power of two that brings the largest |weight| of layer k (all members) below 2^13
  // the fused one-workgroup-per-tile MLP (ani_kernels_mlpf.hip): weight stream and constants per split arithmetic
  // ([0] three bf16 planes, [1] two fp16 planes), built for the AEV layout of the epoch (fused_mask)
  struct Fused {
    unsigned char* stream = nullptr;
    float* consts = nullptr;
    long long ppm = 0;   // pieces per member
    int cpm = 0;         // constants (floats) per member
  } fu[4];   // [arithmetic + 2 * generation]: generation 0 = the 32-rows-per-wave kernel's stream order, 1 = the 16-row kernel's
  int fused_shape = -1;
};
inline MlpArith planes_arith(int i) { return i == 0 ? MLP_BF16X3 : MLP_F16X2; }

// ani_set_option (ani_hip_options.cpp: one table row per name).  Lifetime: the handle's; a value holds until it is set again.
struct Options {
  int prune = 1;          // "prune_absent_species"
  int mlp_pipeline = 0;   // "mlp_pipeline": 1 = large systems run all MLP layers as one launch of persistent workgroups
                          // (two-term arithmetic, shapes off the fused kernel).  Off since round 4: one run of the test suite in
                          // three returned a stale tile at 60 000 atoms (tests/test_hip_properties.py) -- an experiment, not a default
                          // with per-tile dependencies, 2 = at any size (measurement knob), 0 = one launch per layer
  int aev_fused = 1;             // "aev_fused": 1 = neighbour compaction inside the forward AEV launch, 0 = its own kernel
  int aev_sym_radial = 1;        // "aev_symmetric_radial": see AevArgs::row_of_atom
  int aev_tickets_min = 40000;   // "aev_tickets_min": launches of fewer rows keep the fixed stride
  int aev_stream_tables = 1;     // "aev_stream_tables": slot words of the angular pair streams from the handle's tables (StreamTab)
  int mlp_fused_sched = 1;   // "mlp_fused_schedule": 1 = static first-fit schedule of the fused launch, 0 = a counter
  int mlp_fused_halves = 1;  // "mlp_fused_halves": 1 = the schedule may cut straggler items in two (sixteen-row kernel),
                             // 0 = whole items only, 2 = every item as two halves (tests, measurements)
  int mlp_fused = 1;   // "mlp_fused": 1 = networks of three hidden layers run as one launch, a 128-row tile per
                       // workgroup with the activations in registers (ani_kernels_mlpf.hip); 0 = the per-layer kernels
  int mlp_fused_gen = 1;    // "mlp_fused_gen": 1 = sixteen rows per wave (ani_kernels_mlpg.hip), 0 = thirty-two (mlpf)
  int mlp_fused_rows = 0;   // "mlp_fused_rows": rows per workgroup of the 16-row kernel: 128, 64, 0 = by size
  int mlp_chain = 1;   // "mlp_chain": 1 = one chained launch for the MLP of small systems, 2 = at any size, 0 = never
  int profiling = 0;      // "profiling": every entry point synchronises its stream before returning
  int dev_overwrite = 0;  // "device_overwrite_forces": ani_compute_full_device writes d_f instead of adding
  int mlp_arith = MLP_BF16X3;  // "mlp_arith" (an MlpArith): how the MLP evaluates its fp32 products (ani_kernels.h); the exact
                               // split is the default, the reduced-precision fp16 split an opt-in -- the mapping of the reference's
                               // TF32 switch (off unless LAMMPS_ANI_ALLOW_TF32, src/ani_csrc/ani.cpp:41-43)
  int rdf_lanes = 16, rdf_lds = 1;   // "rdf_lanes" / "rdf_lds"
  int nbr_onepass = 1, nbr_sorted_rows = 1, nbr_half_cells = 0;   // "nbr_onepass" / "nbr_sorted_rows" / "nbr_half_cells": see NbrBuild
  int reuse_upload = 0;   // "reuse_build_list_upload"
  // "out_force_accumulate": the host entry points ADD the forces into out_force, chunk by chunk through a
  // page-locked buffer of the library, the additions of one chunk beside the copy of the next
  int out_force_accumulate = 0;
};

// Fused MLP (ani_hip_mlp.cpp).  Lifetime: the weight streams per set of species present, the schedule per list epoch.
struct FusedState {
  int mask[4] = {-2, -2, -2, -2};   // active_mask the fused streams of each (arithmetic, generation) were built for
  DevBuf<int> counter;
  DevBuf<int> sched;    // static schedule of the fused launch: items, then offsets (fused_schedule); remade per list epoch
  int sched_key[4] = {-1, -1, -1, -1};   // what it was made for: total tiles, items per tile, problems, bins
  int sched_nitems = 0;      // entries of the schedule in sched (whole items + halves)
  DevBuf<float> gaev_parts;   // fused MLP with (tile, member) work items: every member's own dE/dAEV rows
};

// Stream tables of the AEV kernels (StreamTab in ani_kernels.h; build_stream_tables in ani_hip_model.cpp).  Lifetime: the species
// map they were built for (mask); a re-neighbouring with the same species present leaves them alone.
struct StreamTables {
  int mask = -2;        // active_mask of the build; -2: never built
  int S = 0, nt = 0;    // S = 0: this layout has no tables (three or more species, or a shape off the fast path)
  int tuples = 0;
  size_t nwords_b = 0, nwords_f = 0;
  int builds = 0;       // how often the tables have been built (ani_debug_stream_tables)
  double build_ms = 0;  // host time of the last build, synchronisations included
  DevBuf<int4> desc_b, desc_f;
  DevBuf<unsigned> words_b, words_f;
  StreamTab view() const { return StreamTab{desc_b.p, words_b.p, desc_f.p, words_f.p, nt}; }
};

struct DevOut { double *member_energy, *atom_energy_dev, *member_dforce, *atom_force_dev, *summary; };   // model deviation: an armed step's outputs

// Per-call armings (ani_hip_armed.cpp).  Lifetime: a request holds for the next step only; the entry point that takes it clears it.
struct Armed {
  // per-atom virial (ani_request_atom_virial): av_acc is the accumulator of the step being run (cleared by run_step /
  // ani_step_begin, NULL on an unarmed step), split_av the output of an armed split step
  double* av_out = nullptr;
  int av_ncomp = 0;
  void* av_acc = nullptr;
  double* split_av = nullptr;
  int split_av_ncomp = 0;
  DevBuf<float> avir;      // [ntotal][9] accumulator (Hartree) of an armed fp32 step
  DevBuf<double> avir64;   // ... of an fp64 step
  DevBuf<double> avout;    // [ntotal][ncomp] the host entry points' result on the device
  // ensemble model deviation (ani_request_model_deviation): dv_req is the request; dv holds the device outputs of
  // the step being run (all NULL on an unarmed step).  dv_force: the step runs the M extra backward passes; dv_dsq: d_j is formed
  // (folded rows: a ghost fold, or no ghosts); dv_fold: the passes' ghost rows go home through the fold
  DevOut dv_req{}, dv{};
  bool dv_on = false, dv_force = false, dv_dsq = false, dv_fold = false;
  DevBuf<double> gaev_parts64;   // fp64 armed steps: every member's dE/dAEV rows, then their deviations dg_m
  DevBuf<float> dv_fbuf;         // [ntotal][4] force accumulator of a member's pass (fp32)
  DevBuf<double> dv_fbuf64;      // [ntotal][3] ... (fp64)
  DevBuf<double> dv_tmp;         // [3][nlocal]: sum over m of |dF|^2, sigma_E and d for the summary
  DevBuf<double> dv_stage;       // the host entry points' outputs on the device
  DevBuf<double> dv_part;        // [M][kDevEnergyParts] block partials of member_energy
  DevBuf<unsigned> dv_ticket;    // the closing kernel's ticket (zero between launches)
};

// Molecule finder (ani_set_bond_table / ani_find_molecules*, ani_hip_analysis.cpp): the caller's table squared, scratch of the
// kernels (ani_kernels_mol.hip: MolArgs), staging of the host entry.  Lifetime: the table until it is set again, the rest one call.
struct MolFinder {
  bool have_bonds = false;
  DevBuf<double> bond_cut2;           // [S][S]
  DevBuf<int> ints;                   // parent | open_atom | open_root | ovf | comp | cnt
  DevBuf<unsigned long long> words;   // counters | keys
  DevBuf<long long> owner, summary;
  DevBuf<int> out;                    // mol_of_atom | formula rows
};

// Radial distribution functions (ani_rdf_*; ani_kernels_rdf.hip: RdfArgs).  Lifetime: from one ani_rdf_configure to the next.
struct Rdf {
  int npair = 0, nbins = 0;       // npair == 0: nothing configured
  double rmax = 0.0;
  DevBuf<int> ints;                   // slot_of [S][S] | pair_a [npair]
  DevBuf<unsigned long long> words;   // hist [npair][nbins] | centres [npair] | frames
};

// Device-side list build (ani_build_list*): scratch of the cell search.  Lifetime: one build; cap_hint from build to build.
struct NbrBuild {
  int cap_hint = 0;   // the longest list of the build before sizes the rows of the next
  DevBuf<int> ovf;
  DevBuf<float4> xq;
  DevBuf<int> cell_id, cell_count, cell_start, cursor, order;
  DevBuf<double> xs;
};

// Host staging of the host-pointer entry points.  Lifetime: the handle's (page-locked memory, made at first use).
struct HostStaging {
  std::vector<int> species32;
  double* pinned_ev = nullptr;  // page-locked {energy, virial[9], error word} of a host-pointer step (launch_step_tail)
  int* pinned_ints = nullptr;   // page-locked host words for small read-backs that ride on a later synchronisation
  double* stage_force = nullptr;   // option out_force_accumulate
  size_t stage_force_cap = 0;
  static constexpr int kForceChunks = 16;
  unsigned* stage_flags = nullptr;          // page-locked: chunk c of the step has landed when stage_flags[c] == copy_epoch
  DevBuf<unsigned long long> copy_ctr;      // workgroups through with chunk c, over all steps (launch_copy_out)
  unsigned copy_epoch = 0;
  unsigned long long step = 0;         // stamp of the host-pointer steps (launch_step_tail)
  const double* x64_from = nullptr;   // ani_build_list has just uploaded these coordinates into x64: the step that follows reuses them
  std::vector<int> half_num, half_j;
};

// Phase timing (ani_phase_timing / ani_phase_times).  Lifetime: from ani_phase_timing(1) until it is read.
struct PhaseTiming {
  bool on = false;
  // one set of 6 events per timed step, recorded on the compute stream without synchronising; elapsed times are
  // resolved lazily in ani_phase_times() so the timed region of a benchmark is not perturbed
  std::vector<hipEvent_t> evt_pool;
  size_t evt_used = 0;
  hipEvent_t* evt = nullptr;
  double phase_ms[5] = {0, 0, 0, 0, 0};   // aev_fwd, mlp, aev_bwd, other, nbr_compact
  int phase_calls = 0;
};

}  // namespace ani_host

using namespace ani;
using namespace ani_host;

struct ani_handle {
  HostModel model;
  AevParams ap{};       // the model's full AEV layout
  AevParams ap_run{};   // the layout the kernels run with this epoch: ap restricted to the species present (set by specialize();
                        // value-initialised: the entry points look at ap_run.full_cap before the first epoch exists)
  SpeciesMap cmap{};  // species -> index among the species present
  int active_mask = -1;
  Options opt;
  FusedState fused;
  StreamTables stab;
  Armed armed;
  MolFinder mol;
  Rdf rdf;
  NbrBuild nb;
  HostStaging host;
  PhaseTiming timing;
  const char* last_mlp_kernel = "";   // ani_last_mlp_kernel: the kernel that ran the MLP of the last step
  const char* last_rep_kernel = "";   // ani_last_repulsion_kernel: the kernel that added the repulsion of the last step
  ChainPlan chain_plan;
  std::vector<int> colmap;  // ap_run column -> ap column
  int device = 0;
  bool use_cuaev = true, use_fullnbr = true, use_single = true;
  hipStream_t stream = nullptr;
  std::string err;
  std::vector<SpeciesNet> nets;

  // list epoch state (valid while ago > 0)
  bool have_list = false;
  // split step (ani_step_*): rows with a ghost among their candidates first in row_list, the others after
  DevBuf<int> row_flag, row_list, row_count;
  int n_boundary = 0;
  bool classes_valid = false;
  int split_phase = 0;          // 0: no split step open, 1: begun, 2: ghosts done
  // the backward pass of the rows without ghosts runs on a low-priority side stream beside the one of the rows with
  // ghosts (both only wait for the MLP): the ghost forces are still done first, and the two kernels share one tail
  hipStream_t side = nullptr;
  hipEvent_t ev_mlp = nullptr, ev_side = nullptr;
  struct { const double* d_x; int eflag_atom, vflag; double *d_f, *d_ev, *d_eatom; } split{};
  int nlocal = 0, ntotal = 0, nrows = 0;
  long long npairs = 0;
  int count[kMaxSpecies] = {0}, row_start[kMaxSpecies] = {0};

  ani_comm* comm = nullptr;   // ani_attach_comm: ghost forces go home on the device (host-pointer entry points)
  int sticky_flags = 0;   // every bit the device error word has ever shown the host (bit 1: LDS capacity, bit 2: MLP wait timeout)
  int max_numneigh = 0;
  DevBuf<int> species, ilist, numneigh, jlist, jraw, nbr_off, row_of_centre, centre_of_row, bucket_info, err_flag;
  DevBuf<int> row_of_atom;   // [ntotal] AEV row of an atom, -1 for atoms that are no centres (AevArgs::row_of_atom)
  DevBuf<unsigned> sym_acc;  // [ntotal] scratch of the list symmetry check (launch_list_symmetry)
  // one-pass list build (launch_nbr_onepass): rows of jraw_stride entries in jraw (0: dense segments), sized from the longest
  // list of the build before
  int jraw_stride = 0;
  // the build in one kernel (launch_nbr_sorted_rows): jlist itself holds rows of jlist_row_stride entries, already grouped by
  // species; the overflow word of that kernel is read behind rebuild()'s own synchronisation (0: dense segments, as ever)
  int jlist_row_stride = 0;
  // ghost fold handed over BEFORE the list it belongs to (ani_stage_ghost_fold): installed by the next list build, its check
  // behind that build's synchronisation
  const int64_t* stage_owner = nullptr;
  const double* stage_shift = nullptr;
  int stage_nghost = -1;
  bool origin_from_box = false;   // ani_build_list*: the caller's bounding box gives the epoch's origin, no kernel
  // ghost fold of the epoch (ani_set_ghost_fold): maps of the caller + the chains of images made from them
  GhostFold fold;
  int fold_nghost = -1;      // -1: none installed (every list build clears it)
  DevBuf<int> fold_head, fold_next, fold_bad;
  bool warned_asymmetric = false;
  bool list_is_ours = false; // the installed list was built by ani_build_list*: symmetric by construction
  bool list_symmetric = true;  // this epoch's list passed the check (or is ours): the symmetric radial collection may run
  DevBuf<int> row_ctr;   // {ticket, waves done} pairs of the fused forward launch, one pair per row range (AevArgs::row_counter)
  DevBuf<float4> xyzs, cl_xyz;
  DevBuf<int4> row_info, cl_hdr;
  DevBuf<int> cl_j;
  int cl_stride = 0;
  DevBuf<double> x64, f64, ev, eatom, virial_acc;
  DevBuf<double> origin;       // [3] the fp32 positions of an epoch are relative to this point (set at its first step)
  bool need_origin = true;
  DevBuf<double> rep_tables, erep;  // optional pairwise repulsion: tables of the model file, energy partial sums
  DevBuf<float> aev, gaev, act, e_rows, fbuf;
  DevBuf<double> aev64, gaev64, act64, e_rows64, fbuf64;  // precision 'double'
  std::vector<std::vector<double*>> Hbuf64;
  std::vector<std::vector<float*>> Hbuf, Gbuf;  // [S][k] pointers into act: stored activations H_k; raw (unmasked) dE/dh_k
  bool arena_valid = false;                     // ... laid out for this epoch's row counts (ensure_arena)
};

#define HIP_TRY(h, expr)                                                                              \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess) {                                                                           \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                                   \
      return ANI_ERR_DEVICE;                                                                          \
    }                                                                                                 \
  } while (0)

namespace ani_host __attribute__((visibility("hidden"))) {
// the functions that cross the ani_hip*.cpp files
int check_args(ani_handle* h, int ntotal, int nlocal, long long npairs, int ago);   // ani_hip.cpp
int upload_model(ani_handle* h);                                                     // ani_hip_model.cpp
int specialize(ani_handle* h, int mask);
int build_stream_tables(ani_handle* h, hipStream_t st);
int compute_mlp(ani_handle* h, hipStream_t st);                                      // ani_hip_mlp.cpp
void free_fused(ani_handle* h, int fi);
const int* forced_fused_split(const char* env, int ntypes, const int* count, int* split);
int rebuild(ani_handle* h, hipStream_t st);                                          // ani_hip_list.cpp
int ingest_list(ani_handle* h, int ntotal, int nlocal, long long npairs, const int* species, const int* ilist, const int* numneigh,
                const int* jlist, hipMemcpyKind kind, hipStream_t st);
int ensure_row_classes(ani_handle* h, hipStream_t st);
// ani_hip_armed.cpp: what an entry point does with the armings of its call
struct DevStage {   // the host entry points: the outputs are staged on the device, then copied into the caller's arrays
  DevOut dev{};   // into dv_stage
  size_t off[5] = {0, 0, 0, 0, 0}, len[5] = {0, 0, 0, 0, 0};
};
double* take_atom_virial(ani_handle* h, int* ncomp);
int atom_virial_begin(ani_handle* h, bool armed);
void atom_virial_out(ani_handle* h, double* d_out, int ncomp, int accumulate, bool fold, hipStream_t st);
bool dv_any(const DevOut& d);
DevOut take_deviation(ani_handle* h);
int deviation_check(ani_handle* h, const DevOut& d, int ntotal, int nlocal, bool device, bool fold);
int deviation_begin(ani_handle* h, const DevOut& d, bool fold);
void deviation_end(ani_handle* h);
int deviation_stage(ani_handle* h, const DevOut& d, int ntotal, int nlocal, DevStage* sg);
int deviation_copy_home(ani_handle* h, const DevOut& d, const DevStage& sg, hipStream_t st);

// ---- ensemble model deviation of an armed step (ani_request_model_deviation) ------------------------------------
// After the step's own kernels: on a force-armed step M passes of the step's backward kernel, pass(m, part_stride, acc) on dg_m into
// the scratch accumulator acc (no virial, atom virial, repulsion or energy: the step's accumulators stay untouched), each followed
// by the kernel that writes member m's rows and adds up |dF|^2; then the closing kernel (member energies, sigma_E, d) and the
// summary.  An energy-only arming costs the closing kernel alone.
template <typename Pass>
int deviation_run(ani_handle* h, Pass&& pass, hipStream_t st) {
  const HostModel& m = h->model;
  const int M = m.M, nl = h->nlocal;
  const bool fp64 = !h->use_single;
  double* dsq = h->armed.dv_dsq ? h->armed.dv_tmp.p : nullptr;
  double* sig = h->armed.dv.summary ? h->armed.dv_tmp.p + (size_t)nl : nullptr;
  double* dd = h->armed.dv.summary ? h->armed.dv_tmp.p + 2 * (size_t)nl : nullptr;
  if (h->armed.dv_force) {
    const long long per = (long long)std::max(h->nrows, 1) * h->ap_run.aev_stride;
    void* acc = fp64 ? static_cast<void*>(h->armed.dv_fbuf64.p) : static_cast<void*>(h->armed.dv_fbuf.p);
    HIP_TRY(h, hipMemsetAsync(acc, 0, (fp64 ? 3 * sizeof(double) : 4 * sizeof(float)) * (size_t)h->ntotal, st));
    const bool fold = h->armed.dv_fold;
    for (int a = 0; a < M; a++) {
      pass(a, per, acc);
      launch_dev_member(acc, fp64, fold ? nl : h->ntotal, nl, a, M, h->armed.dv.member_dforce, dsq, fold ? h->fold_head.p : nullptr,
                        fold ? h->fold_next.p : nullptr, nl, st);
    }
  }
  DevCloseArgs ca{};
  ca.e_rows = fp64 ? static_cast<const void*>(h->e_rows64.p) : static_cast<const void*>(h->e_rows.p);
  ca.M = M; ca.nrows = h->nrows; ca.nrows_ld = h->nrows; ca.nlocal = nl;
  ca.centre_of_row = h->centre_of_row.p; ca.ilist = h->ilist.p; ca.species = h->species.p;
  for (int s = 0; s < m.S; s++) ca.sae[s] = m.sae[s];
  ca.erep = m.has_rep ? h->erep.p : nullptr; ca.nslots = kVirialSlots;
  ca.dsq = dsq;
  ca.member_energy = h->armed.dv.member_energy; ca.atom_energy_dev = h->armed.dv.atom_energy_dev;
  ca.atom_force_dev = dsq ? h->armed.dv.atom_force_dev : nullptr;
  ca.sig = sig; ca.dd = dd;
  ca.partials = h->armed.dv_part.p; ca.ticket = h->armed.dv_ticket.p;
  launch_dev_close(ca, fp64, st);
  if (h->armed.dv.summary) launch_dev_summary(dd, sig, nl, h->armed.dv.summary, st);
  return ANI_OK;
}

// spin on a word the device writes into page-locked host memory; false after 5 s (a stalled device)
template <typename T>
bool wait_host_word(const volatile T* w, T want) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    for (int k = 0; k < 512; k++) {
      if (*w == want) {
        std::atomic_thread_fence(std::memory_order_acquire);
        return true;
      }
      __builtin_ia32_pause();
    }
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) return false;
  }
}
}  // namespace ani_host
