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
#pragma once
#include "qgcm_dev.h"

#define XF_NT 256

struct QgXfParams {
  int ndxr, nxta, nyta, nxpa, nypa, nxtaor, nytaor, nxpaor, nypaor;
  int nxpo, nypo, iocoff, jocoff; // ocean p grid and its offset in the fine atmosphere grid (nxpo = 0: no ocean)
  int cyc_oc, udiff, ndxodd, nijwid;
  int lda, ldta, ldf, ldtf, ldo;  // pitches: atmosphere p / T grid, fine p / T grid, ocean p grid
  const double *pam, *pom;        // layer 1 of the lagged pressures
  double *u1at, *v1at;            // (lda, nypa)
  double *txf, *tyf;              // tauxaor, tauyaor (ldf, nypaor)
  double *wf;                     // wektaor (ldtf, nytaor)
  const double *tbb, *tus, *tvs, *tun, *tvn; // transposed weight tables
  double *tauxa, *tauya, *uekat, *vekat, *wekta, *wekpa;
  double *tauxo, *tauyo;
  QgScalars *sca, *sco;           // the atmosphere's / the cyclic ocean's device scalars (sco: or nullptr)
  double hxafac, hxofac, zbfcat, zbfcoc, cdrfaa, cdrfab, qu2faa, qu2fab, uvekfc, hmrdxa, raoro, dxo;
};

// grid: (ceil(nxpa/256), nypa)
__global__ __launch_bounds__(XF_NT) void k_xf_coarse(const QgXfParams P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + 1;
  const int nxpa = P.nxpa, nypa = P.nypa, ld = P.lda;
  if (i > nxpa) return;
  const double *p = P.pam;
  auto A = [&](int ii, int jj) { return p[(long)(jj - 1) * ld + (ii - 1)]; };
  double u, v;
  if (j == 1) {
    u = -P.zbfcat * (A(i, 2) - A(i, 1));
    v = 0.0;
  } else if (j == nypa) {
    u = -P.zbfcat * (A(i, nypa) - A(i, nypa - 1));
    v = 0.0;
  } else {
    const int ic = (i == nxpa) ? 1 : i; // column nxpa is a copy of column 1
    u = -P.hxafac * (A(ic, j + 1) - A(ic, j - 1));
    v = (ic == 1) ? P.hxafac * (A(2, j) - A(nxpa - 1, j)) : P.hxafac * (A(ic + 1, j) - A(ic - 1, j));
  }
  P.u1at[(long)(j - 1) * ld + (i - 1)] = u;
  P.v1at[(long)(j - 1) * ld + (i - 1)] = v;
}

// One fine point (i, j) of the atmosphere's ocean-resolution p grid: velocity (us, vs) -> stress.
__device__ __forceinline__ void xf_point(const QgXfParams &P, int i, int j, double us, double vs) {
  double cdrfac = P.cdrfaa, qu2fac = P.qu2faa;
  const int io = i - P.iocoff, jo = j - P.jocoff;
  if (P.udiff && io >= 1 && io <= P.nxpo && jo >= 1 && jo <= P.nypo) {
    const int nxpo = P.nxpo, nypo = P.nypo, ld = P.ldo;
    const double *p = P.pom;
    auto O = [&](int ii, int jj) { return p[(long)(jj - 1) * ld + (ii - 1)]; };
    double u1oc, v1oc = 0.0; // (v1ator is unchanged on the zonal boundaries: subtracting 0 changes no bit)
    if (jo == 1) u1oc = -P.zbfcoc * (O(io, 2) - O(io, 1));
    else if (jo == nypo) u1oc = -P.zbfcoc * (O(io, nypo) - O(io, nypo - 1));
    else if (io == 1) {
      if (P.cyc_oc) {
        u1oc = -P.hxofac * (O(1, jo + 1) - O(1, jo - 1));
        v1oc = P.hxofac * (O(2, jo) - O(nxpo - 1, jo));
      } else {
        u1oc = 0.0;
        v1oc = P.zbfcoc * (O(2, jo) - O(1, jo));
      }
    } else if (io == nxpo) {
      if (P.cyc_oc) {
        u1oc = -P.hxofac * (O(nxpo, jo + 1) - O(nxpo, jo - 1));
        v1oc = P.hxofac * (O(2, jo) - O(nxpo - 1, jo));
      } else {
        u1oc = 0.0;
        v1oc = P.zbfcoc * (O(nxpo, jo) - O(nxpo - 1, jo));
      }
    } else {
      u1oc = -P.hxofac * (O(io, jo + 1) - O(io, jo - 1));
      v1oc = P.hxofac * (O(io + 1, jo) - O(io - 1, jo));
    }
    us = us - u1oc;
    vs = vs - v1oc;
    cdrfac = P.cdrfab;
    qu2fac = P.qu2fab;
  }
  const double scasqd = -0.5 + 0.5 * sqrt(1.0 + qu2fac * (us * us + vs * vs));
  const double scashr = sqrt(scasqd);
  const double cdochi = cdrfac * scashr / (1.0 + scasqd);
  const long o = (long)(j - 1) * P.ldf + (i - 1);
  P.txf[o] = cdochi * (us - scashr * vs);
  P.tyf[o] = cdochi * (vs + scashr * us);
}

// grid: (ceil(nxta/XF_CX), nyta): one workgroup per XF_CX zonally adjacent coarse T cells (ic, jc).  A thread owns one
// fine point (ii, jj) of a cell, keeps that point's 16 (+16 next to a zonal boundary) weights in registers and walks
// the workgroup's cells with them, so a weight is fetched once per XF_CX cells; the cells' 16-point neighbourhoods of
// u1at / v1at sit in LDS (one wave-uniform read per term).  With one cell per workgroup the weight reads from L2 -
// 256 bytes per fine point against 16 stored - bound the kernel (profiles/xforc.log).
#define XF_CX 8
static_assert(XF_CX * 32 == XF_NT, "one thread gathers one of the 32 neighbourhood values of one cell");
__global__ __launch_bounds__(XF_NT) void k_xf_fine(const QgXfParams P) {
  __shared__ double dat[XF_CX][32]; // per cell udat(1..16), vdat(1..16)
  const int ic0 = blockIdx.x * XF_CX + 1, jc = blockIdx.y + 1, tid = threadIdx.x;
  const int ndxr = P.ndxr, nxta = P.nxta, nyta = P.nyta, ld = P.lda;
  const int ncell = (nxta - ic0 + 1 < XF_CX) ? nxta - ic0 + 1 : XF_CX;
  {
    const int c = tid >> 5, t = tid & 31;
    if (c < ncell) {
      const int ic = ic0 + c, k = t & 15, q = k & 3, jd = (k >> 2) - 1;
      // cyclic column subscripts icm1, ic, ic+1, icp2
      const int col = q == 0 ? 1 + (ic - 2 + nxta) % nxta : q == 1 ? ic : q == 2 ? ic + 1 : 1 + (ic + 1) % nxta;
      const bool isv = t >= 16;
      double val;
      if (jc == 1 && jd == -1) val = isv ? P.u1at[col - 1] : 0.0;                               // southern padding
      else if (jc == nyta && jd == 2) val = isv ? P.u1at[(long)(P.nypa - 1) * ld + col - 1] : 0.0; // northern padding
      else val = (isv ? P.v1at : P.u1at)[(long)(jc + jd - 1) * ld + col - 1];
      dat[c][t] = val;
    }
  }
  __syncthreads();
  const double *tu, *tv;
  int njj = ndxr;
  if (jc == 1) { tu = P.tus; tv = P.tvs; }
  else if (jc == nyta) { tu = P.tun; tv = P.tvn; njj = ndxr + 1; } // the extra row jj = ndxr
  else { tu = P.tbb; tv = P.tbb; }
  const bool same = tu == tv;
  const int npts = (ndxr + 1) * ndxr; // points per k plane of a table
  const int jfoff = 1 + (jc - 1) * ndxr;
  for (int pt = tid; pt < njj * ndxr; pt += XF_NT) {
    const int jj = pt / ndxr, ii = pt - jj * ndxr;
    double wu[16], wv[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) wu[k] = tu[k * npts + pt];
#pragma unroll
    for (int k = 0; k < 16; ++k) wv[k] = same ? wu[k] : tv[k * npts + pt];
    for (int c = 0; c < ncell; ++c) {
      double us = 0.0, vs = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        us = us + dat[c][k] * wu[k];
        vs = vs + dat[c][16 + k] * wv[k];
      }
      const int i = 1 + (ic0 + c - 1) * ndxr + ii, j = jfoff + jj;
      xf_point(P, i, j, us, vs);
      if (i == 1) xf_point(P, P.nxpaor, j, us, vs); // fine column nxpaor takes the velocity of column 1
    }
  }
}

// grid: (ceil(nxpa/256), nypa)
__global__ __launch_bounds__(XF_NT) void k_xf_atm(const QgXfParams P) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, ja = blockIdx.y + 1;
  if (ia > P.nxpa) return;
  const int ndxr = P.ndxr, ldf = P.ldf;
  const int joff = 1 + (ja - 1) * ndxr;
  {
    const long o = (long)(joff - 1) * ldf + (long)(ia - 1) * ndxr;
    P.tauxa[(long)(ja - 1) * P.lda + (ia - 1)] = P.txf[o];
    P.tauya[(long)(ja - 1) * P.lda + (ia - 1)] = P.tyf[o];
  }
  if (ia <= P.nxta) { // vekat(nxta, nypa): taux along the zonal side of the cell
    const double *t = P.txf + (long)(joff - 1) * ldf + (long)(ia - 1) * ndxr;
    double s = 0.5 * t[0];
    for (int i = 1; i < ndxr; ++i) s = s + t[i];
    s = s + 0.5 * t[ndxr];
    P.vekat[(long)(ja - 1) * P.ldta + (ia - 1)] = P.uvekfc * s;
  }
  if (ja <= P.nyta) { // uekat(nxpa, nyta): tauy along the meridional side; uekat(nxpa, ja) = uekat(1, ja)
    const int ic = (ia == P.nxpa) ? 1 : ia;
    const double *t = P.tyf + (long)(joff - 1) * ldf + (long)(ic - 1) * ndxr;
    double s = 0.5 * t[0];
    for (int j = 1; j < ndxr; ++j) s = s + t[(long)j * ldf];
    s = s + 0.5 * t[(long)ndxr * ldf];
    P.uekat[(long)(ja - 1) * P.lda + (ia - 1)] = -P.uvekfc * s;
  }
}

// grid: (ceil(nxta/256), nyta)
__global__ __launch_bounds__(XF_NT) void k_xf_wekta(const QgXfParams P) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, ja = blockIdx.y + 1;
  if (ia > P.nxta) return;
  const double *ue = P.uekat + (long)(ja - 1) * P.lda + (ia - 1);
  const double *ve = P.vekat + (long)(ja - 1) * P.ldta + (ia - 1);
  P.wekta[(long)(ja - 1) * P.ldta + (ia - 1)] = -P.hmrdxa * (ue[1] - ue[0] + ve[P.ldta] - ve[0]);
}

// grid: (ceil(nxtaor/256), nytaor)
__global__ __launch_bounds__(XF_NT) void k_xf_wektaor(const QgXfParams P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + 1;
  if (i > P.nxtaor) return;
  const int ld = P.ldf;
  const long o = (long)(j - 1) * ld + (i - 1); // (i, j); (i+1, j) = o+1; (i, j+1) = o+ld
  const double *tx = P.txf, *ty = P.tyf;
  P.wf[(long)(j - 1) * P.ldtf + (i - 1)] =
      P.hxofac * (ty[o + 1] + ty[o + ld + 1] - (ty[o] + ty[o + ld]) + tx[o] + tx[o + 1] - (tx[o + ld] + tx[o + ld + 1]));
}

// grid: (ceil(nxpa/64), nypa)
__global__ __launch_bounds__(64) void k_xf_wekpa(const QgXfParams P) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, ja = blockIdx.y + 1;
  if (ia > P.nxpa) return;
  const int ndxr = P.ndxr, nijwid = P.nijwid, nxtaor = P.nxtaor;
  auto wt = [&](int d) { return P.ndxodd ? ((d == 0 || d == ndxr) ? 0.5 : 1.0) : (d == ndxr ? 0.0 : 1.0); };
  const int jbeg = (ja - 1) * ndxr - (ndxr - 1) / 2;
  const int jlo = jbeg > 1 ? jbeg : 1;
  const int jhi = (jbeg + nijwid - 1 < P.nytaor) ? jbeg + nijwid - 1 : P.nytaor;
  const int ibeg = (ia - 1) * ndxr - (ndxr - 1) / 2;
  double wsum = 0.0, wtasum = 0.0;
  for (int j = jlo; j <= jhi; ++j) {
    const double wtj = wt(j - jbeg);
    const double *row = P.wf + (long)(j - 1) * P.ldtf;
    // eight loads in flight, then the sums in the reference's order (d = i - ibeg)
    for (int d0 = 0; d0 < nijwid; d0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int it = ibeg + d0 + u - 1; // 0-based cyclic column: it = 1 + mod(i-1+nxtaor, nxtaor)
        it = it < 0 ? it + nxtaor : (it >= nxtaor ? it - nxtaor : it);
        v[u] = d0 + u < nijwid ? row[it] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (d0 + u < nijwid) {
          const double w = wt(d0 + u) * wtj;
          wsum = wsum + w;
          wtasum = wtasum + w * v[u];
        }
    }
  }
  P.wekpa[(long)(ja - 1) * P.lda + (ia - 1)] = wtasum / wsum;
}

// grid: (ceil(nxpo/256), nypo)
__global__ __launch_bounds__(XF_NT) void k_xf_tauo(const QgXfParams P) {
  const int io = blockIdx.x * blockDim.x + threadIdx.x + 1, jo = blockIdx.y + 1;
  if (io > P.nxpo) return;
  const long f = (long)(P.jocoff + jo - 1) * P.ldf + (P.iocoff + io - 1), o = (long)(jo - 1) * P.ldo + (io - 1);
  P.tauxo[o] = P.raoro * P.txf[f];
  P.tauyo[o] = P.raoro * P.tyf[f];
}

// One workgroup of 256.  Sums 0, 1: the atmosphere's southern / northern line (fine tauxaor rows jsou, jnor; odd ndxr:
// the pairs with rows jsou+1, jnor-1); sums 2, 3: the cyclic ocean's (tauxo rows 1+2, nypo-1+nypo).  Trapezoid end
// weights.  Fixed order: thread-strided along the row, wave butterfly, waves left to right.
__global__ __launch_bounds__(XF_NT) void k_xf_lines(const QgXfParams P) {
  __shared__ double red[4][XF_NT / 64];
  const int tid = threadIdx.x, ndxr = P.ndxr;
  const int jsou = 1 + ndxr / 2, jnor = P.nypaor - ndxr / 2;
  const bool oc = P.sco != nullptr;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 1 + tid; i <= P.nxpaor; i += XF_NT) {
    const double w = (i == 1 || i == P.nxpaor) ? 0.5 : 1.0;
    const double *c = P.txf + (i - 1);
    double a = c[(long)(jsou - 1) * P.ldf], b = c[(long)(jnor - 1) * P.ldf];
    if (P.ndxodd) {
      a = a + c[(long)jsou * P.ldf];
      b = b + c[(long)(jnor - 2) * P.ldf];
    }
    s[0] += w * a;
    s[1] += w * b;
  }
  if (oc)
    for (int i = 1 + tid; i <= P.nxpo; i += XF_NT) {
      const double w = (i == 1 || i == P.nxpo) ? 0.5 : 1.0;
      const double *c = P.tauxo + (i - 1);
      s[2] += w * (c[0] + c[P.ldo]);
      s[3] += w * (c[(long)(P.nypo - 2) * P.ldo] + c[(long)(P.nypo - 1) * P.ldo]);
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int v = 0; v < 4; ++v) s[v] += __shfl_xor(s[v], off);
  if ((tid & 63) == 0)
#pragma unroll
    for (int v = 0; v < 4; ++v) red[v][tid >> 6] = s[v];
  __syncthreads();
  if (tid == 0) {
    double t[4];
    for (int v = 0; v < 4; ++v) {
      t[v] = 0.0;
      for (int w = 0; w < XF_NT / 64; ++w) t[v] += red[v][w];
    }
    const double fa = P.ndxodd ? 0.5 * P.dxo : P.dxo;
    P.sca->txisoc = fa * t[0];
    P.sca->txinoc = fa * t[1];
    if (oc) {
      P.sco->txisoc = 0.5 * P.dxo * t[2];
      P.sco->txinoc = 0.5 * P.dxo * t[3];
    }
  }
}

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
