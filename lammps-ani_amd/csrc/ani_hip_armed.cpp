// ani_hip_armed.cpp — what is armed for one call: per-atom virial and ensemble model deviation.  Internal: see ani_handle.h.
#include "ani_handle.h"

namespace ani_host __attribute__((visibility("hidden"))) {
// an entry point takes the arming (it holds for this one call); out == NULL: unarmed
double* take_atom_virial(ani_handle* h, int* ncomp) {
  double* out = h ? h->armed.av_out : nullptr;
  *ncomp = h ? h->armed.av_ncomp : 0;
  if (h) { h->armed.av_out = nullptr; h->armed.av_ncomp = 0; }
  return out;
}

// the accumulator of the step about to run (grown like the force buffers; cleared inside the step), or none
int atom_virial_begin(ani_handle* h, bool armed) {
  h->armed.av_acc = nullptr;
  if (!armed) return ANI_OK;
  const size_t n = (size_t)std::max(h->ntotal, 1) * 9;
  if (h->use_single) {
    HIP_TRY(h, h->armed.avir.reserve(n));
    h->armed.av_acc = h->armed.avir.p;
  } else {
    HIP_TRY(h, h->armed.avir64.reserve(n));
    h->armed.av_acc = h->armed.avir64.p;
  }
  return ANI_OK;
}

// accumulator -> d_out[rows][ncomp] (kcal/mol, LAMMPS order); a whole-step device call folds the images of an installed ghost fold
void atom_virial_out(ani_handle* h, double* d_out, int ncomp, int accumulate, bool fold, hipStream_t st) {
  const bool f = fold && h->fold_nghost >= 0 && h->use_single;
  launch_atom_virial(h->armed.av_acc, !h->use_single, f ? h->nlocal : h->ntotal, ncomp, d_out, accumulate, f ? h->fold_head.p : nullptr,
                     f ? h->fold_next.p : nullptr, h->nlocal, st);
}

bool dv_any(const DevOut& d) { return d.member_energy || d.atom_energy_dev || d.member_dforce || d.atom_force_dev || d.summary; }
static bool dv_force_outputs(const DevOut& d) { return d.member_dforce || d.atom_force_dev || d.summary; }
static bool dv_folded_outputs(const DevOut& d) { return d.atom_force_dev || d.summary; }

// an entry point takes the arming (it holds for this one call)
DevOut take_deviation(ani_handle* h) {
  const DevOut d = h ? h->armed.dv_req : DevOut{};
  if (h) h->armed.dv_req = DevOut{};
  return d;
}

// the contract checks of an armed call, before it enqueues any work.  fold: the call will run with a ghost fold installed
int deviation_check(ani_handle* h, const DevOut& d, int ntotal, int nlocal, bool device, bool fold) {
  if (!dv_any(d)) return ANI_OK;
  if (!device && h->comm && dv_force_outputs(d)) {
    h->err = "ani_request_model_deviation: the host entry points cannot return force deviations with a communicator attached "
             "(ani_attach_comm): there is no 3M-wide reverse exchange; detach it or use ani_compute_full_device with a ghost fold";
    return ANI_ERR_ARG;
  }
  if (dv_folded_outputs(d) && ntotal != nlocal && !(device && fold && h->use_single)) {
    h->err = "ani_request_model_deviation: atom_force_dev and summary need the ghost rows folded into their owners; this call has "
             "ghost atoms and no ghost fold (ani_set_ghost_fold: ani_compute_full_device, fp32)";
    return ANI_ERR_ARG;
  }
  return ANI_OK;
}

// the armed step about to run: its device outputs and scratch (grown like the force buffers)
int deviation_begin(ani_handle* h, const DevOut& d, bool fold) {
  h->armed.dv = d;
  h->armed.dv_on = dv_any(d);
  h->armed.dv_force = dv_force_outputs(d);
  h->armed.dv_dsq = dv_folded_outputs(d);
  h->armed.dv_fold = fold && h->fold_nghost >= 0 && h->use_single;
  if (!h->armed.dv_on) return ANI_OK;
  if (h->armed.dv_force) {
    if (h->use_single) HIP_TRY(h, h->armed.dv_fbuf.reserve((size_t)std::max(h->ntotal, 1) * 4));
    else HIP_TRY(h, h->armed.dv_fbuf64.reserve((size_t)std::max(h->ntotal, 1) * 3));
  }
  if (h->armed.dv_dsq) HIP_TRY(h, h->armed.dv_tmp.reserve((size_t)std::max(h->nlocal, 1) * 3));
  HIP_TRY(h, h->armed.dv_part.reserve((size_t)h->model.M * kDevEnergyParts));
  HIP_TRY(h, h->armed.dv_ticket.reserve(1, true));
  return ANI_OK;
}

void deviation_end(ani_handle* h) {
  h->armed.dv = DevOut{};
  h->armed.dv_on = h->armed.dv_force = h->armed.dv_dsq = h->armed.dv_fold = false;
}

int deviation_stage(ani_handle* h, const DevOut& d, int ntotal, int nlocal, DevStage* sg) {
  if (!dv_any(d)) return ANI_OK;
  const size_t M = (size_t)h->model.M;
  const size_t len[5] = {M, (size_t)nlocal, (size_t)ntotal * M * 3, (size_t)nlocal, 4};
  size_t tot = 0;
  for (int k = 0; k < 5; k++) { sg->off[k] = tot; sg->len[k] = len[k]; tot += len[k]; }
  HIP_TRY(h, h->armed.dv_stage.reserve(tot));
  double* b = h->armed.dv_stage.p;
  sg->dev.member_energy = d.member_energy ? b + sg->off[0] : nullptr;
  sg->dev.atom_energy_dev = d.atom_energy_dev ? b + sg->off[1] : nullptr;
  sg->dev.member_dforce = d.member_dforce ? b + sg->off[2] : nullptr;
  sg->dev.atom_force_dev = d.atom_force_dev ? b + sg->off[3] : nullptr;
  sg->dev.summary = d.summary ? b + sg->off[4] : nullptr;
  return ANI_OK;
}
int deviation_copy_home(ani_handle* h, const DevOut& d, const DevStage& sg, hipStream_t st) {
  double* const host[5] = {d.member_energy, d.atom_energy_dev, d.member_dforce, d.atom_force_dev, d.summary};
  for (int k = 0; k < 5; k++)
    if (host[k] && sg.len[k])
      HIP_TRY(h, hipMemcpyAsync(host[k], h->armed.dv_stage.p + sg.off[k], sizeof(double) * sg.len[k], hipMemcpyDeviceToHost, st));
  return ANI_OK;
}
}  // namespace ani_host

extern "C" {
// ---- per-atom virial (ani_request_atom_virial) ----------------------------------------------------------------
int ani_request_atom_virial(ani_handle* h, double* out, int ncomp) {
  if (!h) return ANI_ERR_ARG;
  h->armed.av_out = nullptr;
  h->armed.av_ncomp = 0;
  if (!out) return ANI_OK;
  if (ncomp != 6 && ncomp != 9) {
    h->err = "ani_request_atom_virial: ncomp must be 6 (vatom) or 9 (cvatom), got " + std::to_string(ncomp);
    return ANI_ERR_ARG;
  }
  h->armed.av_out = out;
  h->armed.av_ncomp = ncomp;
  return ANI_OK;
}

int ani_request_model_deviation(ani_handle* h, double* member_energy, double* atom_energy_dev, double* member_dforce,
                                double* atom_force_dev, double* summary) {
  if (!h) return ANI_ERR_ARG;
  h->armed.dv_req = DevOut{};
  const DevOut d{member_energy, atom_energy_dev, member_dforce, atom_force_dev, summary};
  if (!dv_any(d)) return ANI_OK;
  if (h->model.M < 2) {
    h->err = "ani_request_model_deviation: needs an ensemble of at least 2 members, the handle uses " + std::to_string(h->model.M);
    return ANI_ERR_ARG;
  }
  h->armed.dv_req = d;
  return ANI_OK;
}
}  // extern "C"
