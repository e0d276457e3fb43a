// ani_kernels_md_protocol.hip — the centre of mass, momentum and angular momentum of the owned atoms and the kernel that removes
// them or recentres (include/ani_md_protocol.h)
#include "ani_md_device.h"

#include "../../include/ani_md_protocol.h"

namespace {

static_assert(ANI_MD_COM_ZERO + 2 == ANI_MD_COM_NREC, "the finish kernel writes the whole record");

constexpr int COM_NSUM = 17;   // M, Sd[3], P[3], Sl[3], S_ab[6], non-finite atoms

// the finish of a sum of block partials in the order of nh_chain_kernel; every thread of the one workgroup has the result
__device__ __forceinline__ double finish_sum(const double* __restrict__ part, int npart, double* red) {
  double a = 0.0;
  for (int b = threadIdx.x; b < npart; b += 256) a += part[b];
  return block_sum_fixed(a, red);
}

// launch 1 of the sample: work[s * nblk + block] = the block's part of sum s
__global__ __launch_bounds__(256) void com_partials_kernel(const double* __restrict__ x, const int* __restrict__ image,
                                                           const double* __restrict__ v, const double* __restrict__ mass, int n, double r0,
                                                           double r1, double r2, double L0, double L1, double L2,
                                                           const double* __restrict__ box_dev, int pmask, double* __restrict__ work) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x, nblk = gridDim.x;
  double q[COM_NSUM];
#pragma unroll
  for (int s = 0; s < COM_NSUM; s++) q[s] = 0.0;
  if (i < n) {
    const Box3 b = box_now(L0, L1, L2, box_dev);
    const double ref[3] = {r0, r1, r2};
    const double m = mass[i];
    double d[3], w[3], md[3];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double xk = x[3 * (size_t)i + k];
      d[k] = (image ? unwrapped(xk, image[3 * (size_t)i + k], b.len[k], (pmask >> k) & 1) : xk) - ref[k];
      w[k] = v[3 * (size_t)i + k];
      md[k] = m * d[k];
      fin = fin && finite_d(d[k]) && finite_d(w[k]);
    }
    q[0] = m;
#pragma unroll
    for (int k = 0; k < 3; k++) { q[1 + k] = md[k]; q[4 + k] = m * w[k]; }
    q[7] = m * (d[1] * w[2] - d[2] * w[1]);
    q[8] = m * (d[2] * w[0] - d[0] * w[2]);
    q[9] = m * (d[0] * w[1] - d[1] * w[0]);
    q[10] = md[0] * d[0]; q[11] = md[1] * d[1]; q[12] = md[2] * d[2];
    q[13] = md[0] * d[1]; q[14] = md[0] * d[2]; q[15] = md[1] * d[2];
    q[16] = fin ? 0.0 : 1.0;
  }
#pragma unroll
  for (int s = 0; s < COM_NSUM; s++) {
    const double sum = block_sum_fixed(q[s], red);
    if (threadIdx.x == 0) work[(size_t)s * nblk + blockIdx.x] = sum;
  }
}

// launch 2: one workgroup finishes the sums, thread 0 writes the record
__global__ __launch_bounds__(256) void com_finish_kernel(const double* __restrict__ work, int nblk, int n, double r0, double r1, double r2,
                                                         double* __restrict__ rec) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  double S[COM_NSUM];
  for (int s = 0; s < COM_NSUM; s++) S[s] = finish_sum(work + (size_t)s * nblk, nblk, red);
  if (threadIdx.x != 0) return;
  const double M = S[0], ref[3] = {r0, r1, r2};
  const double c[3] = {S[1] / M, S[2] / M, S[3] / M}, P[3] = {S[4], S[5], S[6]};
  rec[ANI_MD_COM_MASS] = M;
  for (int k = 0; k < 3; k++) {
    rec[ANI_MD_COM_XCM + k] = ref[k] + c[k];
    rec[ANI_MD_COM_VCM + k] = P[k] / M;
  }
  const double L[3] = {S[7] - (c[1] * P[2] - c[2] * P[1]), S[8] - (c[2] * P[0] - c[0] * P[2]), S[9] - (c[0] * P[1] - c[1] * P[0])};
  const double Cxx = S[10] - M * c[0] * c[0], Cyy = S[11] - M * c[1] * c[1], Czz = S[12] - M * c[2] * c[2];
  const double Cxy = S[13] - M * c[0] * c[1], Cxz = S[14] - M * c[0] * c[2], Cyz = S[15] - M * c[1] * c[2];
  const double Ixx = Cyy + Czz, Iyy = Cxx + Czz, Izz = Cxx + Cyy, Ixy = -Cxy, Ixz = -Cxz, Iyz = -Cyz;
  const double I[6] = {Ixx, Iyy, Izz, Ixy, Ixz, Iyz};
  for (int k = 0; k < 3; k++) rec[ANI_MD_COM_ANGMOM + k] = L[k];
  for (int k = 0; k < 6; k++) rec[ANI_MD_COM_INERTIA + k] = I[k];
  // the cofactors of the symmetric matrix: adj(I) is symmetric as well
  const double Axx = Iyy * Izz - Iyz * Iyz, Ayy = Ixx * Izz - Ixz * Ixz, Azz = Ixx * Iyy - Ixy * Ixy;
  const double Axy = Ixz * Iyz - Ixy * Izz, Axz = Ixy * Iyz - Ixz * Iyy, Ayz = Ixy * Ixz - Ixx * Iyz;
  const double det = (Ixx * Axx + Ixy * Axy) + Ixz * Axz;
  const double tr3 = ((Ixx + Iyy) + Izz) / 3.0;
  const bool singular = n < 2 || fabs(det) <= 1e-12 * ((tr3 * tr3) * tr3);   // one atom: the tensor is rounding noise
  double w[3] = {0.0, 0.0, 0.0};
  if (!singular) {
    w[0] = ((Axx * L[0] + Axy * L[1]) + Axz * L[2]) / det;
    w[1] = ((Axy * L[0] + Ayy * L[1]) + Ayz * L[2]) / det;
    w[2] = ((Axz * L[0] + Ayz * L[1]) + Azz * L[2]) / det;
  }
  for (int k = 0; k < 3; k++) rec[ANI_MD_COM_OMEGA + k] = w[k];
  rec[ANI_MD_COM_SINGULAR] = singular ? 1.0 : 0.0;
  rec[ANI_MD_COM_NONFINITE] = S[16];
  rec[ANI_MD_COM_COUNT] = (double)n;
  rec[ANI_MD_COM_ZERO] = 0.0;
  rec[ANI_MD_COM_ZERO + 1] = 0.0;
}

__global__ __launch_bounds__(256) void com_apply_kernel(double* __restrict__ x, double* __restrict__ v, const int* __restrict__ image, int n,
                                                        const double* __restrict__ rec, int flags, double t0, double t1, double t2,
                                                        int dim_mask, double L0, double L1, double L2, const double* __restrict__ box_dev,
                                                        int pmask, const double* __restrict__ xb, double* __restrict__ d2max) {
#pragma clang fp contract(off)
  if (rec[ANI_MD_COM_NONFINITE] != 0.0) return;      // the whole grid alike
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool recenter = (flags & ANI_MD_COM_FLAG_RECENTER) != 0;
  double d2 = 0.0;
  if (i < n) {
    double xk[3], vk[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { xk[k] = x[3 * (size_t)i + k]; vk[k] = v[3 * (size_t)i + k]; }
    if (flags & ANI_MD_COM_FLAG_LINEAR) {
#pragma unroll
      for (int k = 0; k < 3; k++) vk[k] = vk[k] - rec[ANI_MD_COM_VCM + k];
    }
    if (flags & ANI_MD_COM_FLAG_ANGULAR) {
      const Box3 b = box_now(L0, L1, L2, box_dev);
      double r[3], w[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        r[k] = (image ? unwrapped(xk[k], image[3 * (size_t)i + k], b.len[k], (pmask >> k) & 1) : xk[k]) - rec[ANI_MD_COM_XCM + k];
        w[k] = rec[ANI_MD_COM_OMEGA + k];
      }
      vk[0] = vk[0] - (w[1] * r[2] - w[2] * r[1]);
      vk[1] = vk[1] - (w[2] * r[0] - w[0] * r[2]);
      vk[2] = vk[2] - (w[0] * r[1] - w[1] * r[0]);
    }
    if (flags & (ANI_MD_COM_FLAG_LINEAR | ANI_MD_COM_FLAG_ANGULAR)) {
#pragma unroll
      for (int k = 0; k < 3; k++) v[3 * (size_t)i + k] = vk[k];
    }
    if (recenter) {
      const double target[3] = {t0, t1, t2};
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if ((dim_mask >> k) & 1) {
          xk[k] = xk[k] + (target[k] - rec[ANI_MD_COM_XCM + k]);
          x[3 * (size_t)i + k] = xk[k];
        }
        if (xb) {
          const double d = xk[k] - xb[3 * (size_t)i + k];
          d2 = d2 + d * d;
        }
      }
    }
  }
  if (recenter && xb) fold_d2max(d2, d2max);
}

const double kZero3[3] = {0.0, 0.0, 0.0};

}  // namespace

extern "C" {

int ani_md_com_work_size(int n) { return COM_NSUM * nblocks(n); }

int ani_md_com_sample(const double* x, const int* image, const double* v, const double* mass, int n, const double* ref3,
                      const double* len3, const double* box_dev, int periodic_mask, double* work, double* record, void* stream) {
  if (n <= 0) return 0;
  if (!x || !v || !mass || !ref3 || !work || !record || (image && periodic_mask && !len3 && !box_dev)) return (int)hipErrorInvalidValue;
  const double* l = len3 ? len3 : kZero3;
  const int nblk = nblocks(n);
  enqueue(com_partials_kernel, dim3(nblk), 256, stream, x, image, v, mass, n, ref3[0], ref3[1], ref3[2], l[0], l[1], l[2], box_dev,
          periodic_mask, work);
  return launch(com_finish_kernel, dim3(1), 256, stream, (const double*)work, nblk, n, ref3[0], ref3[1], ref3[2], record);
}

int ani_md_com_apply(double* x, double* v, const int* image, int n, const double* record, int flags, const double* target3,
                     int dim_mask, const double* len3, const double* box_dev, int periodic_mask, const double* x_built,
                     double* d2max, void* stream) {
  if (n <= 0 || !(flags & 7)) return 0;
  const bool recenter = (flags & ANI_MD_COM_FLAG_RECENTER) != 0, angular = (flags & ANI_MD_COM_FLAG_ANGULAR) != 0;
  if (!x || !v || !record || (recenter && !target3) || (x_built && !d2max) ||
      (angular && image && periodic_mask && !len3 && !box_dev))
    return (int)hipErrorInvalidValue;
  const double* l = len3 ? len3 : kZero3;
  const double* t = target3 ? target3 : kZero3;
  return launch(com_apply_kernel, blocks(n), 256, stream, x, v, image, n, record, flags, t[0], t[1], t[2], dim_mask, l[0], l[1], l[2],
                box_dev, periodic_mask, x_built, d2max);
}

}  // extern "C"
