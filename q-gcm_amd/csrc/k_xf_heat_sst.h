// k_xf_heat_sst.h - the heat half of xforc without an ocean: the sibling of k_xf_heat_oc (k_xforc.h) that a
// -Datmos_only build of the reference runs.  Compiled in k_xf_heat_sst.hip only.
#pragma once
#include "qgcm_dev.h"
#include "k_xf_heat_params.h"

// k_xf_heat_sst stands in for k_xf_heat_oc where the reference is built with -Datmos_only: the SST is a prescribed
// field held by the atmosphere handle (P.sstm, pitch P.ldto), read once and never stepped (src/q-gcm.F:753-786).  The
// reference then skips fnetoc and arocsm (src/xfosubs.F:805-812), so there is no fnetoc store, no Dmdown*asto term and
// the cell's arocsm part is written as 0.0: k_xf_heat_atm and k_xf_heat_final follow unchanged and give arocav = 0
// exactly, as the reference's untouched arocsm = 0 does.  Sums as in k_xf_heat_oc: per lane in point order, then the xor
// butterfly.
// grid: (nxaooc, nyaooc), block 64
__global__ __launch_bounds__(64) void k_xf_heat_sst(const QgXfHeatParams P) {
  const int ca = blockIdx.x, cb = blockIdx.y, lane = threadIdx.x, ndxr = P.ndxr;
  const long lda = P.ldta;
  double s[3] = {0.0, 0.0, 0.0}; // the cell's fnetat sum, slhfsm, oradsm
  for (int p = lane; p < ndxr * ndxr; p += 64) {
    const int io = ca * ndxr + p % ndxr, jo = cb * ndxr + p / ndxr; // 0-based SST point
    const int im = P.ix[io] - 1, ip = P.ix[P.nxto + io] - 1, jm = P.iy[jo] - 1, jp = P.iy[P.nyto + jo] - 1;
    const double wmx = P.wx[io], wpx = P.wx[P.nxto + io], wmy = P.wy[jo], wpy = P.wy[P.nyto + jo];
    // bilint's four terms in its order, fmult = 1 (:985-988)
    const double asto = 1.0 * (wmx * wmy * P.astm[jm * lda + im] + wpx * wmy * P.astm[jm * lda + ip] +
                               wmx * wpy * P.astm[jp * lda + im] + wpx * wpy * P.astm[jp * lda + ip]);
    const double sst = P.sstm[(long)jo * P.ldto + io];
    const double ocnrad = P.D0up * sst;          // :800
    const double slhf = P.xlamda * (sst - asto); // :803
    const double atmrad = P.dmdu * asto;         // :815, dmdu = Dmdown - Dmup
    s[0] += P.ocfrac * (ocnrad + atmrad + slhf); // :816-817
    s[1] += slhf;
    s[2] += ocnrad;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_xor(s[q], off);
  if (lane == 0) {
    const int c = cb * P.nxaooc + ca;
    P.cell[c] = s[0];
    P.part[c] = 0.0; // arocsm: never accumulated under atmos_only
    P.part[P.ncell + c] = s[1];
    P.part[2 * P.ncell + c] = s[2];
  }
}
