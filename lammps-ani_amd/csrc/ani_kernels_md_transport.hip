// ani_kernels_md_transport.hip — image flags through the wrap, unwrapped positions, mean-squared displacements and packed
// trajectory frames of the timestep loop (include/ani_md_transport.h)
#include "ani_md_device.h"

#include "../../include/ani_md_transport.h"

namespace {

static_assert(ANI_MD_MSD_NONFINITE + 1 == ANI_MD_MSD_NOUT, "the finish kernel writes the whole row of a group");
static_assert(ANI_MD_MSD_MAXCLASS <= 32, "a group is a bit mask of classes in an int32");

constexpr int MSD_NSUM = 10;   // per class: S2[3], S1[3], Sm[3], non-finite atoms

// wrap_kernel of ani_kernels_md.hip, the same expression and the same two clamps, with the box lengths it removed kept as counts
__global__ __launch_bounds__(256) void wrap_images_kernel(double* __restrict__ x, int* __restrict__ image, int n, double lo0, double lo1,
                                                          double lo2, double l0, double l1, double l2, int pmask) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const int k = t % 3;
  if (!((pmask >> k) & 1)) return;
  const double lo = k == 0 ? lo0 : (k == 1 ? lo1 : lo2), L = k == 0 ? l0 : (k == 1 ? l1 : l2);
  double v = x[t];
  const double q = floor((v - lo) / L);
  v -= q * L;
  int add = (int)q;
  if (v >= lo + L) { v = lo; add += 1; }   // a coordinate that rounds up onto the upper face: it is one more box length away
  if (v < lo) v = lo;                      // a quotient that rounds up to the integer: q already counts that box length
  x[t] = v;
  image[t] += add;
}

__global__ __launch_bounds__(256) void unwrap_kernel(const double* __restrict__ x, const int* __restrict__ image, int n, double L0, double L1,
                                                     double L2, const double* __restrict__ box_dev, int pmask, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const int k = t % 3;
  const Box3 b = box_now(L0, L1, L2, box_dev);
  out[t] = unwrapped(x[t], image[t], b.len[k], (pmask >> k) & 1);
}

// launch 1: work[(c * MSD_NSUM + s) * nblk + block] = the block's part of sum s of class c
__global__ __launch_bounds__(256) void msd_partials_kernel(const double* __restrict__ x, const int* __restrict__ image,
                                                           const double* __restrict__ x0u, const double* __restrict__ mass,
                                                           const int* __restrict__ cls, int n, int nclass, double L0, double L1, double L2,
                                                           const double* __restrict__ box_dev, int pmask, double* __restrict__ work) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x, nblk = gridDim.x;
  const Box3 b = box_now(L0, L1, L2, box_dev);
  int c_own = -1;
  double v[MSD_NSUM];
#pragma unroll
  for (int s = 0; s < MSD_NSUM; s++) v[s] = 0.0;
  if (i < n) {
    c_own = cls[i];
    if (c_own < 0 || c_own >= nclass) c_own = -1;
    const double m = mass[i];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double d = unwrapped(x[3 * (size_t)i + k], image[3 * (size_t)i + k], b.len[k], (pmask >> k) & 1) - x0u[3 * (size_t)i + k];
      v[k] = d * d;
      v[3 + k] = d;
      v[6 + k] = m * d;
      fin = fin && finite_d(d);
    }
    v[9] = fin ? 0.0 : 1.0;
  }
  for (int c = 0; c < nclass; c++) {
    const bool mine = c_own == c;
#pragma unroll
    for (int s = 0; s < MSD_NSUM; s++) {
      const double sum = block_sum_fixed(mine ? v[s] : 0.0, red);
      if (threadIdx.x == 0) work[((size_t)c * MSD_NSUM + s) * nblk + blockIdx.x] = sum;
    }
  }
}

// launch 2: one workgroup; the partials in the strided order of nh_chain_kernel, classes into groups ascending, the outputs
__global__ __launch_bounds__(256) void msd_finish_kernel(const double* __restrict__ work, int nblk, int nclass,
                                                         const int* __restrict__ class_count, const double* __restrict__ class_mass,
                                                         const int* __restrict__ group_mask, int ngroup, double* __restrict__ out,
                                                         double step, double* __restrict__ series_row) {
  __shared__ double red[4];
  __shared__ double cs[ANI_MD_MSD_MAXCLASS * MSD_NSUM];
  for (int c = 0; c < nclass; c++)
    for (int s = 0; s < MSD_NSUM; s++) {
      const double* __restrict__ part = work + ((size_t)c * MSD_NSUM + s) * nblk;
      double a = 0.0;
      for (int p = threadIdx.x; p < nblk; p += 256) a += part[p];
      a = block_sum_fixed(a, red);
      if (threadIdx.x == 0) cs[c * MSD_NSUM + s] = a;
    }
  __syncthreads();
  const int g = threadIdx.x;
  if (g == 0 && series_row) series_row[0] = step;
  if (g >= ngroup) return;
  const unsigned mask = (unsigned)group_mask[g];
  double S[MSD_NSUM], N = 0.0, M = 0.0;
#pragma unroll
  for (int s = 0; s < MSD_NSUM; s++) S[s] = 0.0;
  for (int c = 0; c < nclass; c++) {
    if (!((mask >> c) & 1u)) continue;
#pragma unroll
    for (int s = 0; s < MSD_NSUM; s++) S[s] += cs[c * MSD_NSUM + s];
    N += (double)class_count[c];
    M += class_mass[c];
  }
  double o[ANI_MD_MSD_NOUT];
#pragma unroll
  for (int j = 0; j < ANI_MD_MSD_NOUT; j++) o[j] = 0.0;
  if (N > 0.0) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double s2 = S[k] / N, s1 = S[3 + k] / N, dcm = S[6 + k] / M;
      o[ANI_MD_MSD_MSD + k] = s2;
      o[ANI_MD_MSD_COM + k] = (s2 - (2.0 * dcm) * s1) + dcm * dcm;
      o[ANI_MD_MSD_DCM + k] = dcm;
    }
    o[ANI_MD_MSD_MSD + 3] = (o[ANI_MD_MSD_MSD] + o[ANI_MD_MSD_MSD + 1]) + o[ANI_MD_MSD_MSD + 2];
    o[ANI_MD_MSD_COM + 3] = (o[ANI_MD_MSD_COM] + o[ANI_MD_MSD_COM + 1]) + o[ANI_MD_MSD_COM + 2];
    o[ANI_MD_MSD_NONFINITE] = S[9];
  }
#pragma unroll
  for (int j = 0; j < ANI_MD_MSD_NOUT; j++) {
    out[g * ANI_MD_MSD_NOUT + j] = o[j];
    if (series_row) series_row[1 + g * ANI_MD_MSD_NOUT + j] = o[j];
  }
}

// xyz[k][row[i]] = (float)position; thread 0 writes the cell of the moment
__global__ __launch_bounds__(256) void frame_pack_kernel(const double* __restrict__ x, const int* __restrict__ image, int n,
                                                         const int* __restrict__ row, double lo0, double lo1, double lo2, double L0,
                                                         double L1, double L2, const double* __restrict__ lo_dev,
                                                         const double* __restrict__ box_dev, int pmask, int unwrap,
                                                         float* __restrict__ xyz, double* __restrict__ cell) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const Box3 b = box_now(L0, L1, L2, box_dev);
  if (t == 0) {
    cell[0] = lo_dev ? lo_dev[0] : lo0;
    cell[1] = lo_dev ? lo_dev[1] : lo1;
    cell[2] = lo_dev ? lo_dev[2] : lo2;
    cell[3] = b.len[0];
    cell[4] = b.len[1];
    cell[5] = b.len[2];
  }
  if (t >= 3 * n) return;
  const int i = t / 3, k = t - 3 * i;
  const int r = row[i];
  if (r < 0 || r >= n) return;          // a row that points outside is skipped, never followed
  const double v = unwrap ? unwrapped(x[t], image[t], b.len[k], (pmask >> k) & 1) : x[t];
  xyz[(size_t)k * n + r] = (float)v;
}

const double kZero3[3] = {0.0, 0.0, 0.0};

}  // namespace

extern "C" {

int ani_md_wrap_positions_images(double* x, int* image, int n, const double* lo3, const double* len3, int periodic_mask, void* stream) {
  if (n <= 0 || periodic_mask == 0) return 0;
  if (!x || !image || !lo3 || !len3) return (int)hipErrorInvalidValue;
  return launch(wrap_images_kernel, blocks(3 * n), 256, stream, x, image, n, lo3[0], lo3[1], lo3[2], len3[0], len3[1], len3[2],
                periodic_mask);
}

int ani_md_unwrap(const double* x, const int* image, int n, const double* len3, const double* box_dev, int periodic_mask, double* out,
                  void* stream) {
  if (n <= 0) return 0;
  if (!x || !image || !out || (!len3 && !box_dev)) return (int)hipErrorInvalidValue;
  const double* l = len3 ? len3 : kZero3;
  return launch(unwrap_kernel, blocks(3 * n), 256, stream, x, image, n, l[0], l[1], l[2], box_dev, periodic_mask, out);
}

int ani_md_msd_work_size(int nlocal, int nclass) {
  const int nc = nclass < 1 ? 1 : (nclass > ANI_MD_MSD_MAXCLASS ? ANI_MD_MSD_MAXCLASS : nclass);
  return nc * MSD_NSUM * nblocks(nlocal);
}

int ani_md_msd_sample(const double* x, const int* image, const double* x0u, const double* mass, const int* cls, int n, int nclass,
                      const int* class_count, const double* class_mass, const int* group_mask, int ngroup, const double* len3,
                      const double* box_dev, int periodic_mask, double* work, double* out, double step, double* series_row,
                      void* stream) {
  if (!x || !image || !x0u || !mass || !cls || !class_count || !class_mass || !group_mask || !work || !out || (!len3 && !box_dev) ||
      n <= 0 || nclass < 1 || nclass > ANI_MD_MSD_MAXCLASS || ngroup < 1 || ngroup > ANI_MD_MSD_MAXGROUP)
    return (int)hipErrorInvalidValue;
  const double* l = len3 ? len3 : kZero3;
  const int nblk = nblocks(n);
  enqueue(msd_partials_kernel, dim3(nblk), 256, stream, x, image, x0u, mass, cls, n, nclass, l[0], l[1], l[2], box_dev, periodic_mask,
          work);
  return launch(msd_finish_kernel, dim3(1), 256, stream, (const double*)work, nblk, nclass, class_count, class_mass, group_mask, ngroup,
                out, step, series_row);
}

int ani_md_frame_pack(const double* x, const int* image, int n, const int* row, const double* lo3, const double* len3,
                      const double* lo_dev, const double* box_dev, int periodic_mask, int unwrap, float* xyz, double* cell,
                      void* stream) {
  if (!x || (unwrap && !image) || !row || !xyz || !cell || (!len3 && !box_dev) || (!lo3 && !lo_dev) || n <= 0)
    return (int)hipErrorInvalidValue;
  const double* l = len3 ? len3 : kZero3;
  const double* o = lo3 ? lo3 : kZero3;
  return launch(frame_pack_kernel, blocks(3 * n), 256, stream, x, image, n, row, o[0], o[1], o[2], l[0], l[1], l[2], lo_dev, box_dev,
                periodic_mask, unwrap ? 1 : 0, xyz, cell);
}

}  // extern "C"
