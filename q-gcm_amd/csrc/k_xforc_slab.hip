// k_xforc_slab.hip - the kernels of xforc on a y-slab ocean (k_xforc_slab.h) as a translation unit, and so a
// device code object, of its own, for the reason k_tend_rows.hip gives: qgcm_hip.hip compiles to the device code it
// compiled to before these kernels existed.
#define QG_XFORC_SLAB_KERNELS
#include "k_xforc_slab.h"

// the ocean side of the momentum half after tauxo / tauyo / wekto: wekpo on the local rows and, cyclic, the line integrals
hipError_t qg_launch_xf_slab_ocean(hipStream_t st, const QgXfSlabParams &P) {
  hipLaunchKernelGGL(k_xf_wekpo_slab, dim3((P.nx + XFS_NT - 1) / XFS_NT, P.nyl), dim3(XFS_NT), 0, st, P);
  if (P.cyc) hipLaunchKernelGGL(k_xf_lines_oc_slab, dim3(1), dim3(XFS_NT), 0, st, P);
  return hipGetLastError();
}

hipError_t qg_launch_xf_heat_oc_slab(hipStream_t st, const QgXfHeatSlabParams &S) {
  hipLaunchKernelGGL(k_xf_heat_oc_slab, dim3(S.h.nxaooc, S.h.nyaooc), dim3(64), 0, st, S);
  return hipGetLastError();
}

hipError_t qg_launch_xf_heat_combine(hipStream_t st, const double *gath, int nranks, int ncell, double *cell, double *part) {
  hipLaunchKernelGGL(k_xf_heat_combine, dim3((ncell + XFS_NT - 1) / XFS_NT), dim3(XFS_NT), 0, st, gath, nranks, ncell, cell, part);
  return hipGetLastError();
}
