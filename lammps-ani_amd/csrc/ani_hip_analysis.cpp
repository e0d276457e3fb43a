// ani_hip_analysis.cpp — analysis over the installed list: molecule finder and ani_rdf_*.  Internal: see ani_handle.h.
#include "ani_handle.h"

extern "C" {
// ---- molecule finder (ani_set_bond_table, ani_find_molecules*): see include/ani_hip.h ---------------------------------------
int ani_set_bond_table(ani_handle* h, const double* cut, int nspecies) {
  if (!h) return ANI_ERR_ARG;
  if (!cut) { h->mol.have_bonds = false; return ANI_OK; }   // cleared
  const int S = h->model.S;
  if (nspecies != S) {
    h->err = "ani_set_bond_table: nspecies = " + std::to_string(nspecies) + ", the model has " + std::to_string(S) + " species";
    return ANI_ERR_ARG;
  }
  const double rmax = std::min(h->model.Rcr, h->model.Rca);
  std::vector<double> c2((size_t)S * S);
  for (int a = 0; a < S; a++)
    for (int b = 0; b < S; b++) {
      const double v = cut[a * S + b], w = cut[b * S + a];
      const std::string pair = "[" + h->model.symbols[a] + "][" + h->model.symbols[b] + "]";
      if (v != v) { h->err = "ani_set_bond_table: entry " + pair + " is not a number"; return ANI_ERR_ARG; }
      if (!(v == w) && !(v <= 0 && w <= 0)) { h->err = "ani_set_bond_table: the table is asymmetric at " + pair; return ANI_ERR_ARG; }
      if (v > rmax) {
        h->err = "ani_set_bond_table: entry " + pair + " = " + std::to_string(v) + " A is above the cutoff " + std::to_string(rmax) +
                 " A (the list is only complete inside the force cutoff)";
        return ANI_ERR_ARG;
      }
      c2[(size_t)a * S + b] = v > 0 ? v * v : -1.0;
    }
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipDeviceSynchronize());   // a call that still reads the table before it is replaced (rare: set-up time)
  HIP_TRY(h, h->mol.bond_cut2.reserve(c2.size()));
  HIP_TRY(h, hipMemcpy(h->mol.bond_cut2.p, c2.data(), sizeof(double) * c2.size(), hipMemcpyHostToDevice));
  h->mol.have_bonds = true;
  return ANI_OK;
}

static int find_molecules_args(ani_handle* h, int ntotal, int nlocal, int formula_cap) {
  if (!h) return ANI_ERR_ARG;
  if (!h->use_fullnbr) { h->err = "ani_find_molecules: the handle was created for half lists (use_fullnbr = 0)"; return ANI_ERR_ARG; }
  if (!h->mol.have_bonds) { h->err = "ani_find_molecules: no bond table is set (ani_set_bond_table)"; return ANI_ERR_ARG; }
  if (!h->have_list) { h->err = "ani_find_molecules: no neighbour list is installed (a call with ago == 0, or ani_build_list*)"; return ANI_ERR_ARG; }
  if (ntotal != h->ntotal || nlocal != h->nlocal) {
    h->err = "ani_find_molecules: ntotal / nlocal = " + std::to_string(ntotal) + " / " + std::to_string(nlocal) +
             " differ from the installed list's " + std::to_string(h->ntotal) + " / " + std::to_string(h->nlocal);
    return ANI_ERR_ARG;
  }
  if (formula_cap < 0) { h->err = "ani_find_molecules: negative formula_cap"; return ANI_ERR_ARG; }
  if (nlocal >= (1 << 29)) { h->err = "ani_find_molecules: more than 2^29 owned atoms per rank is not supported"; return ANI_ERR_ARG; }
  return ANI_OK;
}

int ani_find_molecules_device(ani_handle* h, int ntotal, int nlocal, const double* d_x, const int64_t* d_owner, int* d_mol_of_atom,
                              int* d_formula, int formula_cap, int64_t* d_summary, void* stream) {
  const int rc = find_molecules_args(h, ntotal, nlocal, formula_cap);
  if (rc) return rc;
  if (!d_x) { h->err = "ani_find_molecules: null positions"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int S = h->model.S;
  MolArgs a{};
  a.nlocal = nlocal; a.ntotal = ntotal; a.S = S;
  a.table_size = 64;
  while (a.table_size < 2 * nlocal) a.table_size *= 2;
  a.ovf_cap = std::max(nlocal, 1);
  const size_t n1 = (size_t)std::max(nlocal, 1);
  HIP_TRY(h, h->mol.ints.reserve(4 * n1 + n1 * S + (size_t)a.table_size));
  HIP_TRY(h, h->mol.words.reserve((size_t)kMolCounters + (size_t)a.table_size));
  a.parent = h->mol.ints.p; a.open_atom = a.parent + n1; a.open_root = a.open_atom + n1; a.ovf = a.open_root + n1;
  a.comp = a.ovf + n1; a.cnt = a.comp + n1 * S;
  a.counters = h->mol.words.p; a.keys = a.counters + kMolCounters;
  a.ilist = h->ilist.p; a.nbr_off = h->nbr_off.p; a.numneigh = h->numneigh.p; a.jlist = h->jlist.p; a.species = h->species.p;
  a.x = d_x; a.cut2 = h->mol.bond_cut2.p;
  static_assert(sizeof(long long) == sizeof(int64_t), "owner indices are 64-bit");
  a.owner = d_owner ? reinterpret_cast<const long long*>(d_owner) : (h->fold_nghost >= 0 ? h->fold.owner : nullptr);
  a.mol_of_atom = d_mol_of_atom; a.formula = d_formula; a.formula_cap = formula_cap;
  a.summary = reinterpret_cast<long long*>(d_summary);
  TraceRange tr("ani: molecule finder");
  launch_find_molecules(a, st);
  HIP_TRY(h, take_launch_error());
  return ANI_OK;
}

int ani_find_molecules(ani_handle* h, int ntotal, int nlocal, const double* coordinates, const int64_t* owner, int* mol_of_atom,
                       int* formula, int formula_cap, int64_t* summary) {
  int rc = find_molecules_args(h, ntotal, nlocal, formula_cap);
  if (rc) return rc;
  if (!coordinates) { h->err = "ani_find_molecules: null positions"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int S = h->model.S, W = S + 1, ng = ntotal - nlocal;
  const size_t nrow = formula ? (size_t)formula_cap : 0;
  HIP_TRY(h, h->x64.reserve((size_t)std::max(ntotal, 1) * 3));
  h->host.x64_from = nullptr;   // the staging array no longer holds what ani_build_list uploaded
  HIP_TRY(h, hipMemcpyAsync(h->x64.p, coordinates, sizeof(double) * 3 * (size_t)ntotal, hipMemcpyHostToDevice, st));
  if (owner && ng > 0) {
    HIP_TRY(h, h->mol.owner.reserve((size_t)ng));
    HIP_TRY(h, hipMemcpyAsync(h->mol.owner.p, owner, sizeof(int64_t) * (size_t)ng, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(h, h->mol.out.reserve((size_t)std::max(nlocal, 1) + nrow * W));
  HIP_TRY(h, h->mol.summary.reserve(6));
  int* d_formula = formula ? h->mol.out.p + std::max(nlocal, 1) : nullptr;
  rc = ani_find_molecules_device(h, ntotal, nlocal, h->x64.p, owner && ng > 0 ? reinterpret_cast<const int64_t*>(h->mol.owner.p) : nullptr,
                                 mol_of_atom ? h->mol.out.p : nullptr, d_formula, formula_cap,
                                 reinterpret_cast<int64_t*>(h->mol.summary.p), st);
  if (rc) return rc;
  long long sum[6];
  if (mol_of_atom && nlocal > 0) HIP_TRY(h, hipMemcpyAsync(mol_of_atom, h->mol.out.p, sizeof(int) * (size_t)nlocal, hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipMemcpyAsync(sum, h->mol.summary.p, sizeof(sum), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));
  if (summary) for (int k = 0; k < 6; k++) summary[k] = sum[k];
  const size_t rows = (size_t)std::min<long long>(sum[1], (long long)nrow);
  if (rows) {
    HIP_TRY(h, hipMemcpy(formula, d_formula, sizeof(int) * rows * W, hipMemcpyDeviceToHost));
    // ascending, lexicographically by composition
    std::vector<int> order(rows);
    for (size_t r = 0; r < rows; r++) order[r] = (int)r;
    std::sort(order.begin(), order.end(), [&](int p, int q) {
      return std::lexicographical_compare(formula + (size_t)p * W, formula + (size_t)p * W + S, formula + (size_t)q * W, formula + (size_t)q * W + S);
    });
    std::vector<int> sorted(rows * W);
    for (size_t r = 0; r < rows; r++) std::copy(formula + (size_t)order[r] * W, formula + (size_t)order[r] * W + W, sorted.begin() + r * W);
    std::copy(sorted.begin(), sorted.end(), formula);
  }
  if (formula && sum[1] > (long long)formula_cap) {
    h->err = "ani_find_molecules: " + std::to_string(sum[1]) + " distinct compositions, formula_cap is " + std::to_string(formula_cap);
    return ANI_ERR_CAPACITY;
  }
  return ANI_OK;
}

// ---- radial distribution functions (ani_rdf_*): see include/ani_hip.h -------------------------------------------------------
int ani_rdf_configure(ani_handle* h, int nbins, double rmax, const int* pairs, int npair) {
  if (!h) return ANI_ERR_ARG;
  if (!h->use_fullnbr) { h->err = "ani_rdf_configure: the handle was created for half lists (use_fullnbr = 0)"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  if (!pairs || npair == 0) {   // cleared
    HIP_TRY(h, hipDeviceSynchronize());
    h->rdf.npair = 0;
    return ANI_OK;
  }
  const int S = h->model.S;
  if (npair < 0) { h->err = "ani_rdf_configure: npair = " + std::to_string(npair) + " is negative"; return ANI_ERR_ARG; }
  if (nbins < 1 || nbins > kRdfMaxBins) {
    h->err = "ani_rdf_configure: nbins = " + std::to_string(nbins) + " is outside [1, " + std::to_string(kRdfMaxBins) + "]";
    return ANI_ERR_ARG;
  }
  if (!(rmax > 0.0) || !std::isfinite(rmax)) { h->err = "ani_rdf_configure: rmax = " + std::to_string(rmax) + " is not a positive finite number"; return ANI_ERR_ARG; }
  if (rmax > h->model.Rcr) {
    h->err = "ani_rdf_configure: rmax = " + std::to_string(rmax) + " A is above the radial cutoff " + std::to_string(h->model.Rcr) +
             " A (the list is only complete inside the force cutoff)";
    return ANI_ERR_ARG;
  }
  std::vector<int> tab((size_t)S * S + (size_t)npair, -1);
  for (int p = 0; p < npair; p++) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    for (int v : {a, b})
      if (v < 0 || v >= S) {
        h->err = "ani_rdf_configure: pair " + std::to_string(p) + " names species " + std::to_string(v) + ", outside [0, " + std::to_string(S) + ")";
        return ANI_ERR_ARG;
      }
    if (tab[(size_t)a * S + b] >= 0) {
      h->err = "ani_rdf_configure: the ordered pair (" + h->model.symbols[a] + ", " + h->model.symbols[b] + ") is listed twice (pairs " +
               std::to_string(tab[(size_t)a * S + b]) + " and " + std::to_string(p) + ")";
      return ANI_ERR_ARG;
    }
    tab[(size_t)a * S + b] = p;
    tab[(size_t)S * S + p] = a;
  }
  // accumulations still in flight write the words that are replaced here (rare: set-up time)
  HIP_TRY(h, hipDeviceSynchronize());
  h->rdf.npair = 0;   // a failure below leaves nothing configured
  const size_t words = (size_t)npair * nbins + (size_t)npair + 1;
  HIP_TRY(h, h->rdf.ints.reserve(tab.size()));
  HIP_TRY(h, h->rdf.words.reserve(words));
  HIP_TRY(h, hipMemcpy(h->rdf.ints.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemset(h->rdf.words.p, 0, sizeof(unsigned long long) * words));
  HIP_TRY(h, hipStreamSynchronize(nullptr));   // the handle's streams do not wait for the null stream
  h->rdf.npair = npair; h->rdf.nbins = nbins; h->rdf.rmax = rmax;
  return ANI_OK;
}

static int rdf_accumulate_args(ani_handle* h, int ntotal, int nlocal) {
  if (!h) return ANI_ERR_ARG;
  if (!h->use_fullnbr) { h->err = "ani_rdf_accumulate: the handle was created for half lists (use_fullnbr = 0)"; return ANI_ERR_ARG; }
  if (h->rdf.npair == 0) { h->err = "ani_rdf_accumulate: nothing is configured (ani_rdf_configure)"; return ANI_ERR_ARG; }
  if (!h->have_list) { h->err = "ani_rdf_accumulate: no neighbour list is installed (a call with ago == 0, or ani_build_list*)"; return ANI_ERR_ARG; }
  if (ntotal != h->ntotal || nlocal != h->nlocal) {
    h->err = "ani_rdf_accumulate: ntotal / nlocal = " + std::to_string(ntotal) + " / " + std::to_string(nlocal) +
             " differ from the installed list's " + std::to_string(h->ntotal) + " / " + std::to_string(h->nlocal);
    return ANI_ERR_ARG;
  }
  return ANI_OK;
}

int ani_rdf_accumulate_device(ani_handle* h, int ntotal, int nlocal, const double* d_x, void* stream) {
  const int rc = rdf_accumulate_args(h, ntotal, nlocal);
  if (rc) return rc;
  if (!d_x) { h->err = "ani_rdf_accumulate: null positions"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  const int S = h->model.S;
  RdfArgs a{};
  a.nlocal = nlocal; a.ntotal = ntotal; a.S = S;
  a.ilist = h->ilist.p; a.nbr_off = h->nbr_off.p; a.numneigh = h->numneigh.p; a.jlist = h->jlist.p; a.species = h->species.p;
  a.x = d_x;
  a.slot_of = h->rdf.ints.p; a.pair_a = h->rdf.ints.p + (size_t)S * S;
  a.npair = h->rdf.npair; a.nbins = h->rdf.nbins;
  a.rmax = h->rdf.rmax; a.inv_dr = (double)h->rdf.nbins / h->rdf.rmax;
  a.hist = h->rdf.words.p; a.centres = a.hist + (size_t)a.npair * a.nbins; a.frames = a.centres + a.npair;
  TraceRange tr("ani: rdf sample");
  launch_rdf_accumulate(a, h->opt.rdf_lanes, h->opt.rdf_lds, (hipStream_t)stream);
  HIP_TRY(h, take_launch_error());
  return ANI_OK;
}

int ani_rdf_accumulate(ani_handle* h, int ntotal, int nlocal, const double* coordinates) {
  int rc = rdf_accumulate_args(h, ntotal, nlocal);
  if (rc) return rc;
  if (!coordinates) { h->err = "ani_rdf_accumulate: null positions"; return ANI_ERR_ARG; }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  HIP_TRY(h, h->x64.reserve((size_t)std::max(ntotal, 1) * 3));
  h->host.x64_from = nullptr;   // the staging array no longer holds what ani_build_list uploaded
  HIP_TRY(h, hipMemcpyAsync(h->x64.p, coordinates, sizeof(double) * 3 * (size_t)ntotal, hipMemcpyHostToDevice, st));
  rc = ani_rdf_accumulate_device(h, ntotal, nlocal, h->x64.p, st);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(st));
  return ANI_OK;
}

int ani_rdf_read(ani_handle* h, uint64_t* counts, uint64_t* centres, uint64_t* frames, int reset) {
  if (!h) return ANI_ERR_ARG;
  if (h->rdf.npair == 0) { h->err = "ani_rdf_read: nothing is configured (ani_rdf_configure)"; return ANI_ERR_ARG; }
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the accumulators are 64-bit words");
  HIP_TRY(h, hipSetDevice(h->device));
  // the device entry runs on the caller's streams: everything that writes the accumulators is waited for
  HIP_TRY(h, hipDeviceSynchronize());
  const size_t nh = (size_t)h->rdf.npair * h->rdf.nbins, np = (size_t)h->rdf.npair;
  const unsigned long long* w = h->rdf.words.p;
  if (counts) HIP_TRY(h, hipMemcpy(counts, w, sizeof(uint64_t) * nh, hipMemcpyDeviceToHost));
  if (centres) HIP_TRY(h, hipMemcpy(centres, w + nh, sizeof(uint64_t) * np, hipMemcpyDeviceToHost));
  if (frames) HIP_TRY(h, hipMemcpy(frames, w + nh + np, sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (reset) {
    HIP_TRY(h, hipMemset(h->rdf.words.p, 0, sizeof(unsigned long long) * (nh + np + 1)));
    HIP_TRY(h, hipStreamSynchronize(nullptr));
  }
  return ANI_OK;
}
}  // extern "C"
