// What another handle may know of an SQ8 index (csrc/sq8.hip): csrc/ivf.hip lays an inverted-file overlay over its resident int8
// rows and csrc/ivf_sq8.hip scans them list by list.  The score rule lives here once, so that every kernel that scores SQ8 rows
// returns the bits include/vrag_amd.h ("SQ8 dense rows") states.
#pragma once
#include <hip/hip_runtime.h>

namespace vrag {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// score = (float)idot * (s_q * s_r): the conversion, the scale product, the final product -- three roundings, no fused step
__device__ __forceinline__ float sq8_score(int idot, float sq, float sr) {
  const float scale = __fmul_rn(sq, sr);
  return __fmul_rn((float)idot, scale);
}

// The rows' device addresses, their layout and how many are in place, read under the index's lock.  codes [size][stride] int8
// (stride = dim rounded up to 16 bytes, pad codes zero), scales [size] fp32.  The addresses are fixed for the index's lifetime.
struct Sq8View {
  const signed char* codes;
  const float* scales;
  int stride, dim, device;
  long long size;
};

// fp32 queries [nq][dim] on the device -> codes [nq][stride] and scales [nq] by the rows' rule (sq8_query_kernel); no argument
// is checked, the launch's status is returned.
hipError_t launch_sq8_query(const float* queries, int nq, int dim, int stride, signed char* qcodes, float* qscales, hipStream_t st);

}  // namespace vrag

struct vrag_sq8_index;
namespace vrag {
Sq8View sq8_index_view(vrag_sq8_index* ix);
}  // namespace vrag
