// k_xforc_slab.hip - the kernels of xforc on a y-slab ocean (k_xforc_slab.h) as a translation unit, and so a
// device code object, of its own, for the reason k_tend_rows.hip gives: qgcm_hip.hip compiles to the device code it
// compiled to before these kernels existed.
#define QG_XFORC_SLAB_KERNELS
#include "k_xforc_slab.h"

// the ocean side of the momentum half after tauxo / tauyo / wekto: wekpo on the local rows and, cyclic, the line integrals
// (P.lines: which; a middle slab of a banded channel forms none)
hipError_t qg_launch_xf_slab_ocean(hipStream_t st, const QgXfSlabParams &P) {
  hipLaunchKernelGGL(k_xf_wekpo_slab, dim3((P.nx + XFS_NT - 1) / XFS_NT, P.nyl), dim3(XFS_NT), 0, st, P);
  if (P.cyc && P.lines) hipLaunchKernelGGL(k_xf_lines_oc_slab, dim3(1), dim3(XFS_NT), 0, st, P);
  return hipGetLastError();
}

hipError_t qg_launch_xf_heat_oc_slab(hipStream_t st, const QgXfHeatSlabParams &S) {
  hipLaunchKernelGGL(k_xf_heat_oc_slab, dim3(S.h.nxaooc, S.h.nyaooc), dim3(64), 0, st, S);
  return hipGetLastError();
}

hipError_t qg_launch_xf_heat_combine(hipStream_t st, const double *gath, int nranks, int ncell, long stride, long off, double *cell,
                                     double *part) {
  hipLaunchKernelGGL(k_xf_heat_combine, dim3((ncell + XFS_NT - 1) / XFS_NT), dim3(XFS_NT), 0, st, gath, nranks, ncell, stride, off, cell,
                     part);
  return hipGetLastError();
}

// ---- banded mode ---------------------------------------------------------------------------------------------
// the fine stress on the cell rows c0 .. c1: u1at, v1at on the coarse rows their neighbourhoods reach, then k_xf_fine
hipError_t qg_launch_xf_win_fine(hipStream_t st, const QgXfParams &P, int c0, int c1) {
  const dim3 b(XF_NT);
  const int j0 = c0 > 1 ? c0 - 1 : 1, j1 = c1 + 2 < P.nypa ? c1 + 2 : P.nypa;
  QgXfWin W = {j0, 0, 0};
  hipLaunchKernelGGL(k_xf_coarse_win, dim3((P.nxpa + XF_NT - 1) / XF_NT, j1 - j0 + 1), b, 0, st, P, W);
  W.j0 = c0;
  hipLaunchKernelGGL(k_xf_fine_win, dim3((P.nxta + XF_CX - 1) / XF_CX, c1 - c0 + 1), b, 0, st, P, W);
  return hipGetLastError();
}

// the band a0 .. a1 of atmosphere p rows from the fine stress: tauxa, tauya, vekat on a0 .. min(a1 + 1, nypa) (wekta at
// a1 reads vekat at a1 + 1), uekat and wekta on a0 .. min(a1, nyta), wektaor on the fine T rows t0 .. t1 that wekpa on
// a0 .. a1 reads; lines: the atmosphere's line sums to form (QgXfWin); stage: wekpa by k_xf_wekpa_stage
hipError_t qg_launch_xf_wekpa_stage(hipStream_t st, const QgXfParams &P, int ja0, int nrow); // k_xf_wekpa_stage.hip
hipError_t qg_launch_xf_win_band(hipStream_t st, const QgXfParams &P, int a0, int a1, int t0, int t1, int lines, bool stage) {
  const dim3 b(XF_NT);
  const int ae = a1 + 1 < P.nypa ? a1 + 1 : P.nypa, au = a1 < P.nyta ? a1 : P.nyta;
  QgXfWin W = {a0, au, lines};
  hipLaunchKernelGGL(k_xf_atm_win, dim3((P.nxpa + XF_NT - 1) / XF_NT, ae - a0 + 1), b, 0, st, P, W);
  if (au >= a0) hipLaunchKernelGGL(k_xf_wekta_win, dim3((P.nxta + XF_NT - 1) / XF_NT, au - a0 + 1), b, 0, st, P, W);
  W.j0 = t0;
  hipLaunchKernelGGL(k_xf_wektaor_win, dim3((P.nxtaor + XF_NT - 1) / XF_NT, t1 - t0 + 1), b, 0, st, P, W);
  W.j0 = a0;
  if (stage) {
    const hipError_t e = qg_launch_xf_wekpa_stage(st, P, a0, a1 - a0 + 1);
    if (e != hipSuccess) return e;
  } else
    hipLaunchKernelGGL(k_xf_wekpa_win, dim3((P.nxpa + 63) / 64, a1 - a0 + 1), dim3(64), 0, st, P, W);
  if (lines) hipLaunchKernelGGL(k_xf_lines_win, dim3(1), b, 0, st, P, W);
  return hipGetLastError();
}

hipError_t qg_launch_xf_band_pack(hipStream_t st, const QgXfBandMsg &B) {
  hipLaunchKernelGGL(k_xf_band_pack, dim3((B.nxpa + XFS_NT - 1) / XFS_NT, B.nrow, XFB_NF), dim3(XFS_NT), 0, st, B);
  return hipGetLastError();
}

hipError_t qg_launch_xf_band_scatter(hipStream_t st, const QgXfBandMsg &B) {
  hipLaunchKernelGGL(k_xf_band_scatter, dim3((B.nxpa + XFS_NT - 1) / XFS_NT, B.nrow, XFB_NF * B.nranks), dim3(XFS_NT), 0, st, B);
  return hipGetLastError();
}

// ---- tau_udiff -------------------------------------------------------------------------------------------------
hipError_t qg_launch_xf_pom_pack(hipStream_t st, const QgXfPomMsg &M) {
  hipLaunchKernelGGL(k_xf_pom_pack, dim3((M.nxpo + XFS_NT - 1) / XFS_NT, M.nrow), dim3(XFS_NT), 0, st, M);
  return hipGetLastError();
}

hipError_t qg_launch_xf_pom_assemble(hipStream_t st, const QgXfPomMsg &M) {
  hipLaunchKernelGGL(k_xf_pom_assemble, dim3((M.nxpo + XFS_NT - 1) / XFS_NT, M.nrow, M.nranks), dim3(XFS_NT), 0, st, M);
  return hipGetLastError();
}

// ---- owner-computed sums -------------------------------------------------------------------------------------------
hipError_t qg_launch_xf_edge_pack(hipStream_t st, const QgXfEdgeMsg &M) {
  hipLaunchKernelGGL(k_xf_edge_pack, dim3((M.nxpo + XFS_NT - 1) / XFS_NT, 2 * XFE_ROWS), dim3(XFS_NT), 0, st, M);
  return hipGetLastError();
}

hipError_t qg_launch_xf_edge_assemble(hipStream_t st, const QgXfEdgeMsg &M) {
  hipLaunchKernelGGL(k_xf_edge_assemble, dim3((M.nxpo + XFS_NT - 1) / XFS_NT, M.g1 - M.g0 + 1 + 2 * XFE_ROWS), dim3(XFS_NT), 0, st, M);
  return hipGetLastError();
}

// wektaor on the owned fine T rows t0 .. t1 (after qg_launch_xf_win_fine on the plan's one window)
hipError_t qg_launch_xf_sums_wektaor(hipStream_t st, const QgXfParams &P, int t0, int t1) {
  const QgXfWin W = {t0, 0, 0};
  hipLaunchKernelGGL(k_xf_wektaor_win, dim3((P.nxtaor + XF_NT - 1) / XF_NT, t1 - t0 + 1), dim3(XF_NT), 0, st, P, W);
  return hipGetLastError();
}

// the atmosphere's line sums the rank owns, then its samples and partial sums into the message's momentum block
hipError_t qg_launch_xf_sums_part(hipStream_t st, const QgXfParams &P, const QgXfSumMsg &B) {
  const QgXfWin W = {1, 0, B.own & 3};
  if (W.lines) hipLaunchKernelGGL(k_xf_lines_win, dim3(1), dim3(XF_NT), 0, st, P, W);
  hipLaunchKernelGGL(k_xf_sums_atm, dim3((B.nxpa + XFS_NT - 1) / XFS_NT, B.nrow), dim3(XFS_NT), 0, st, B);
  hipLaunchKernelGGL(k_xf_sums_wekpa, dim3((B.nxpa + 63) / 64, B.nrow), dim3(64), 0, st, B);
  return hipGetLastError();
}

hipError_t qg_launch_xf_sums_combine(hipStream_t st, const QgXfSumMsg &B) {
  hipLaunchKernelGGL(k_xf_sums_combine, dim3((B.nxpa + XFS_NT - 1) / XFS_NT, B.nypa), dim3(XFS_NT), 0, st, B);
  return hipGetLastError();
}
