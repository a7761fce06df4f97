// k_tend_rows.hip - the row-band kernel of the 5 km box ocean (k_tend_rows.h) as a translation unit, and so a device
// code object, of its own.  Why: appended to qgcm_hip.hip's code object the two instantiations left every other kernel
// its instruction stream and its place, and yet the unchanged kernels of the 5 km step ran 0.2 - 0.7 us slower per launch
// (DESIGN 3.10).  Built here, qgcm_hip.hip compiles to the device code it compiled to before the kernel existed.
#ifdef QG_STAMPS
#define qg_stamps qg_stamps_rows // (development builds: this code object's own table of phase stamps, read below)
#endif
#include "qgcm_dev.h"
// (the kernel headers also define non-template kernels: qgcm_hip.hip owns those; here they are static and unused - a few dead kernels
//  of some hundred bytes each in this code object, no clash of their host stubs at link time)
#pragma push_macro("__global__")
#undef __global__
#define __global__ static __attribute__((global))
#include "k_tend.h"
#include "k_dst64.h"
#pragma pop_macro("__global__")
#include "k_tend_rows.h"

// zm: the zero-field mask (0 or 3: the instantiations); grid and block follow from the geometry in P
void qg_launch_tend_rows(int zm, hipStream_t st, const QgTendParams &P, const double2 *twid, const double *sintab) {
  constexpr int B = TR_BAND;
  const QgGeom &g = P.g;
  const int nbands = (g.ny - 2 + B - 1) / B;
  const dim3 grid(8 * ((nbands + 7) / 8));
  const int side = P.upd_dpi ? 2 : 0;
  if (zm) hipLaunchKernelGGL((k_tend_rows<3, B, 3>), grid, dim3(TrCfg<B>::NT), 0, st, P.pom, twid, sintab, g.nx, g.ny, g.ldx, side, P);
  else hipLaunchKernelGGL((k_tend_rows<3, B, 0>), grid, dim3(TrCfg<B>::NT), 0, st, P.pom, twid, sintab, g.nx, g.ny, g.ldx, side, P);
}

#ifdef QG_STAMPS
// development builds only (profiles/tools/stamps_band.py): the phase stamps of the last launch of the band kernel
// (TR_STAMP, k_tend_rows.h), laid out as qgcm_hip_debug_stamps lays out qgcm_hip.hip's
extern "C" int qgcm_hip_debug_stamps_rows(long long *out, size_t nbytes) {
  if (nbytes > sizeof(qg_stamps)) nbytes = sizeof(qg_stamps);
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(qg_stamps), nbytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif
