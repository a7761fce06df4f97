// k_xf_wekpa_stage.hip - k_xf_wekpa_stage (k_xf_wekpa_stage.h) as a translation unit, and so a device code
// object, of its own, for the reason k_tend_rows.hip gives: qgcm_hip.hip and k_xforc_slab.hip compile to the device code
// they compiled to before the kernel existed.
#include "k_xf_wekpa_stage.h"

extern "C" int qgcm_hip_xf_wekpa_stage_points(void) { return XFW_G; }

#define XFW_EACH(F) F(4) F(8) F(10) F(12) F(16)
static_assert((XFW_G * XFW_NDXR_MAX + XFW_NT - 1) / XFW_NT <= 16, "the widest instantiation holds a row of XFW_NDXR_MAX");

// once per xforc set-up: the dynamic LDS of the instantiation this ndxr takes, where it passes the default limit
hipError_t qg_setup_xf_wekpa_stage(int ndxr) {
  if (ndxr < 1 || ndxr > XFW_NDXR_MAX) return hipErrorInvalidValue;
  const size_t lds = xfw_lds_bytes(ndxr);
  if (lds <= 64 * 1024) return hipSuccess;
  const int need = xfw_loads(ndxr);
#define XFW_ATTR(U) \
  if (need <= U) return hipFuncSetAttribute((const void *)k_xf_wekpa_stage<U>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  XFW_EACH(XFW_ATTR)
#undef XFW_ATTR
  return hipErrorInvalidValue;
}

// wekpa on the atmosphere p rows ja0 .. ja0 + nrow - 1 (the whole grid: 1, nypa; a band of the slab path: a0, a1 - a0 + 1)
hipError_t qg_launch_xf_wekpa_stage(hipStream_t st, const QgXfParams &P, int ja0, int nrow) {
  if (P.ndxr < 1 || P.ndxr > XFW_NDXR_MAX) return hipErrorInvalidValue;
  const dim3 grid((P.nxpa + XFW_G - 1) / XFW_G, nrow), block(XFW_NT);
  const size_t lds = xfw_lds_bytes(P.ndxr);
  const int need = xfw_loads(P.ndxr);
#define XFW_LAUNCH(U) \
  if (need <= U) { \
    hipLaunchKernelGGL(k_xf_wekpa_stage<U>, grid, block, lds, st, P, ja0); \
    return hipGetLastError(); \
  }
  XFW_EACH(XFW_LAUNCH)
#undef XFW_LAUNCH
  return hipErrorInvalidValue;
}
