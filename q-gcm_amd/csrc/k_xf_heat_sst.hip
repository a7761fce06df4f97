// k_xf_heat_sst.hip - k_xf_heat_sst (k_xf_heat_sst.h) as a translation unit, and so a device code object, of its own, for
// the reason k_tend_rows.hip gives: qgcm_hip.hip compiles to the device code it compiled to before the kernel existed,
// and no kernel of the ocean's step moves inside its code object.
#include "k_xf_heat_sst.h"

hipError_t qg_launch_xf_heat_sst(hipStream_t st, const QgXfHeatParams &P) {
  hipLaunchKernelGGL(k_xf_heat_sst, dim3(P.nxaooc, P.nyaooc), dim3(64), 0, st, P);
  return hipGetLastError();
}
