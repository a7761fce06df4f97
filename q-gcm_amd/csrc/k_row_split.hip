// k_row_split.hip - the kernels of k_row_split.h as a translation unit, and so a device code object, of their own, for
// the reason k_tend_rows.hip gives: qgcm_hip.hip compiles to the device code it compiled to before the kernels existed,
// and no kernel of the existing steps moves inside its code object.
#include "k_row_split.h"

// which: SPLIT_GATHER .. SPLIT_SCATTER; P = S.P in 2 .. 5 (qgcm_hip_row_split)
hipError_t qg_launch_row_split(int which, hipStream_t st, const QgRowSplit &S, int nlayers) {
  const int npts = which == SPLIT_FWD ? S.N / 2 + 1 : which == SPLIT_INV ? S.L / 2 + 1 : S.N;
  const dim3 grid((npts + SPLIT_NT - 1) / SPLIT_NT, S.nrows, nlayers), block(SPLIT_NT);
#define QG_SPLIT(PV)                                                                                      \
  case PV:                                                                                                \
    if (which == SPLIT_GATHER) hipLaunchKernelGGL((k_split_copy<PV, false>), grid, block, 0, st, S);      \
    else if (which == SPLIT_SCATTER) hipLaunchKernelGGL((k_split_copy<PV, true>), grid, block, 0, st, S); \
    else if (which == SPLIT_FWD) hipLaunchKernelGGL((k_split_fwd<PV>), grid, block, 0, st, S);            \
    else hipLaunchKernelGGL((k_split_inv<PV>), grid, block, 0, st, S);                                    \
    break;
  switch (S.P) {
    QG_SPLIT(2) QG_SPLIT(3) QG_SPLIT(4) QG_SPLIT(5)
    default: return hipErrorInvalidValue;
  }
#undef QG_SPLIT
  return hipGetLastError();
}
