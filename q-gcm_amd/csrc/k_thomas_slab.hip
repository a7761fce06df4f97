// k_thomas_slab.hip - the two kernels of a y-slab cut into segments (k_thomas_slab.h) as a translation unit, and so a
// device code object, of their own, for the reason k_tend_rows.hip gives: qgcm_hip.hip compiles to the device code it
// compiled to before they existed, and no kernel of a step that does not use them moves inside its code object.
#include "qgcm_dev.h"
// (k_thomas.h also defines kernels: qgcm_hip.hip owns those; here they are static and unused, as in k_tend_rows.hip)
#pragma push_macro("__global__")
#undef __global__
#define __global__ static __attribute__((global))
#include "k_thomas.h"
#pragma pop_macro("__global__")
#include "k_thomas_slab.h"

// setup: the right-hand-side independent half (once per set of diagonals), else the per-solve half
hipError_t qg_launch_thomas_fold(bool setup, hipStream_t st, const QgThomasFold &F) {
  const dim3 grid((F.nk + 63) / 64, F.nl);
  if (setup) hipLaunchKernelGGL(k_thomas_fold<true>, grid, dim3(64), 0, st, F);
  else hipLaunchKernelGGL(k_thomas_fold<false>, grid, dim3(64), 0, st, F);
  return hipGetLastError();
}

// nslice: slices of THC_UNR * THC_NT / 8 rows that cover the longest segment
hipError_t qg_launch_thomas_corr_slab(hipStream_t st, const QgThomasParams &P, const QgThomasCorr &T, const QgThomasSegRec *segs,
                                      const QgThomasFold &F, int nslice, int nlayers) {
  const size_t lds = sizeof(double) * THC_LDS * P.nranks;
  if (lds > 32 * 1024) { // (more than 31 slabs: beyond the default dynamic-LDS limit of a launch)
    const hipError_t e = hipFuncSetAttribute((const void *)k_thomas_corr_slab, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_thomas_corr_slab, dim3(P.nblk, nlayers, F.S * nslice), dim3(THC_NT), lds, st, P, T, segs, F, nslice);
  return hipGetLastError();
}
