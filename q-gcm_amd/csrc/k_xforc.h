// k_xforc.h - the momentum half of xforc (src/xfosubs.F:137-709 with auvbcu, :997-1234) on the device:
//
//   k_xf_coarse   geostrophic velocity u1at, v1at of pam(:,:,1) at the atmosphere's p points (:182-213)
//   k_xf_fine     per coarse T cell: the bicubic interpolant of u1at, v1at at the cell's ndxr x ndxr ocean-resolution
//                 points (auvbcu; a workgroup walks XF_CX cells), minus the ocean's geostrophic velocity where tau_udiff applies (:244-300), through
//                 the quadratic drag law (:319-353) -> tauxaor, tauyaor.  u1ator / v1ator exist in registers only.
//   k_xf_atm      tauxa, tauya (sample, :362-367), vekat, uekat (side integrals of the fine stress, :377-410)
//   k_xf_wekta    wekta from the divergence of uekat, vekat (:412-415)
//   k_xf_wektaor  Ekman velocity at the fine T points (:425-432)
//   k_xf_wekpa    its weighted box average at the atmosphere's p points (:446-471), summed in the reference's order
//   k_xf_tauo     tauxo, tauyo = raoro * the fine stress above the ocean (:554-559); k_wekto / k_wekpo (k_setup.h) follow
//   k_xf_lines    the stress line integrals txisat, txinat (:493-517) and, cyclic ocean, txisoc, txinoc (:672-683)
//
// Every pointwise expression keeps the reference's operand order (the build has -ffp-contract=off): bitwise the
// reference.  The line integrals are parallel sums with a fixed tree (reproducible, equal to rounding).
// Indices in comments are the reference's 1-based ones.  The weight tables are held transposed,
// tab[k][jj][ii] (jj = 0..ndxr, ii = 0..ndxr-1), so that the lanes of a wave read consecutive doubles of one k plane;
// all workgroups read the same 35 KB (ndxr = 16) plane set, which stays in L2.
// The text of the kernels is k_xforc_rows.inc, which the row-windowed kernels of the banded slab path (k_xforc_slab.h,
// DESIGN 6p) include a second time; here it is compiled for the rows of the whole grid.
#pragma once
#include "k_xforc_rows.h" // QgXfParams, XF_NT, XF_CX, xf_point

#define XF_K(name) name
#define XF_WIN_ARG
#define XF_J0 1
#define XF_JUMAX P.nyta
#define XF_SOUTH true
#define XF_NORTH true
#define XF_LINES_OC P.sco != nullptr
#define XF_WINDOWED 0
#include "k_xforc_rows.inc"
#undef XF_K
#undef XF_WIN_ARG
#undef XF_J0
#undef XF_JUMAX
#undef XF_SOUTH
#undef XF_NORTH
#undef XF_LINES_OC
#undef XF_WINDOWED

// ---- heat half (src/xfosubs.F:711-853, bilint :891-993) -----------------------------------------------------
//   k_xf_heat_oc     one wave per atmosphere cell above the ocean: at each of its ndxr x ndxr ocean T points asto (bilint,
//                    from the host-built index / weight tables; never stored), ocnrad, slhf, atmrad -> fnetoc (pointwise:
//                    bitwise the reference's); the cell's sum of ocfrac*(ocnrad + atmrad + slhf) and its parts of the
//                    arocav / slhfav / oradav sums: per lane in point order, then the xor butterfly (fixed order, no atomics)
//   k_xf_heat_atm    one thread per atmosphere T point: the land value or the cell's sum, then the pointwise tail
//                    (:833-844); per-workgroup partial sums of astm over land (arlaav)
//   k_xf_heat_final  one workgroup: the four monitors
// About 15 MB of traffic at the 961 x 961 ocean (sstm in, fnetoc out): small beside the momentum half.
#include "k_oml.h" // oml_block_sums

#include "k_xf_heat_params.h" // QgXfHeatParams

// grid: (nxaooc, nyaooc), block 64
__global__ __launch_bounds__(64) void k_xf_heat_oc(const QgXfHeatParams P) {
  const int ca = blockIdx.x, cb = blockIdx.y, lane = threadIdx.x, ndxr = P.ndxr;
  const long lda = P.ldta;
  double s[4] = {0.0, 0.0, 0.0, 0.0}; // the cell's fnetat sum, arocsm, slhfsm, oradsm
  for (int p = lane; p < ndxr * ndxr; p += 64) {
    const int io = ca * ndxr + p % ndxr, jo = cb * ndxr + p / ndxr; // 0-based ocean T point
    const int im = P.ix[io] - 1, ip = P.ix[P.nxto + io] - 1, jm = P.iy[jo] - 1, jp = P.iy[P.nyto + jo] - 1;
    const double wmx = P.wx[io], wpx = P.wx[P.nxto + io], wmy = P.wy[jo], wpy = P.wy[P.nyto + jo];
    // bilint's four terms in its order, fmult = 1 (:985-988)
    const double asto = 1.0 * (wmx * wmy * P.astm[jm * lda + im] + wpx * wmy * P.astm[jm * lda + ip] +
                               wmx * wpy * P.astm[jp * lda + im] + wpx * wpy * P.astm[jp * lda + ip]);
    const long o = (long)jo * P.ldto + io;
    const double sst = P.sstm[o];
    const double ocnrad = P.D0up * sst;           // :800
    const double slhf = P.xlamda * (sst - asto);  // :803
    const double atmrad = P.Dmdown * asto;        // :807
    P.fnetoc[o] = -P.fso[jo] - atmrad - ocnrad - slhf; // :810
    const double atmrad2 = P.dmdu * asto;         // :815, dmdu = Dmdown - Dmup
    s[0] += P.ocfrac * (ocnrad + atmrad2 + slhf); // :816-817
    s[1] += atmrad;
    s[2] += slhf;
    s[3] += ocnrad;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_xor(s[q], off);
  if (lane == 0) {
    const int c = cb * P.nxaooc + ca;
    P.cell[c] = s[0];
    P.part[c] = s[1];
    P.part[P.ncell + c] = s[2];
    P.part[2 * P.ncell + c] = s[3];
  }
}

// grid: (ceil(nxta/64), ceil(nyta/4)), block 256 = 64 x 4
__global__ __launch_bounds__(OML_NT) void k_xf_heat_atm(const QgXfHeatParams P) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 64 + (tid & 63) + 1, j = blockIdx.y * 4 + (tid >> 6) + 1;
  double t[1] = {0.0};
  if (i <= P.nxta && j <= P.nyta) {
    const long o = (long)(j - 1) * P.ldta + (i - 1);
    const double am = P.astm[o];
    const int ca = i - P.nx1, cb = j - P.ny1;
    double f;
    if (ca >= 0 && ca < P.nxaooc && cb >= 0 && cb < P.nyaooc) f = P.cell[cb * P.nxaooc + ca]; // :752, 816 (0 + the sum)
    else {
      f = -P.fsa[j - 1] - P.Dmup * am; // :738
      t[0] = am;                       // arlasm: the cells over land (:740, 755)
    }
    const double *p1 = P.pam + (long)(j - 1) * P.lda + (i - 1), *p2 = p1 + P.fstride;
    const long n = P.lda;
    double dt = 0.0;
    if (P.dtop) {
      const double *d = P.dtop + (long)(j - 1) * P.lda + (i - 1);
      dt = d[0] + d[1] + d[n] + d[n + 1];
    }
    f = f - P.fmafac * (p1[0] - p2[0] + p1[1] - p2[1] + p1[n] - p2[n] + p1[n + 1] - p2[n + 1]) - P.fmatop * dt +
        P.hmafac * (P.hmm[o] - P.hmat); // :835-842
    P.fnetat[o] = f;
  }
  oml_block_sums<1>(t, red, tid);
  if (tid == 0) P.part[3 * P.ncell + blockIdx.y * gridDim.x + blockIdx.x] = t[0];
}

// one workgroup of 256
__global__ __launch_bounds__(OML_NT) void k_xf_heat_final(const QgXfHeatParams P) {
  __shared__ double red[16];
  const int tid = threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = tid; k < P.ncell; k += OML_NT) {
    a[0] += P.part[k];
    a[1] += P.part[P.ncell + k];
    a[2] += P.part[2 * P.ncell + k];
  }
  for (int k = tid; k < P.nblkL; k += OML_NT) a[3] += P.part[3 * P.ncell + k];
  oml_block_sums<4>(a, red, tid);
  if (tid == 0) {
    P.scal[0] = P.natlan == 0 ? 0.0 : P.Dmup * a[3] / (double)P.natlan; // arlaav, :761-766
    P.scal[1] = a[1] * P.ocnorm; // slhfav, :850-852
    P.scal[2] = a[2] * P.ocnorm; // oradav
    P.scal[3] = a[0] * P.ocnorm; // arocav
  }
}

// The heat half without an ocean (atmos_only) replaces k_xf_heat_oc by k_xf_heat_sst, which lives in
// k_xf_heat_sst.h / k_xf_heat_sst.hip, a device code object of its own: k_xf_heat_atm and k_xf_heat_final follow it unchanged.
