// k_xforc_rows.h - what the two sets of atmosphere-side kernels of xforc's momentum half share: the parameter struct,
// the stress at one fine point, and the kernels' text itself, k_xforc_rows.inc, which is written once and included by
//
//   k_xforc.h        as the whole-domain kernels k_xf_*: rows 1 .. n of a grid (compiled in qgcm_hip.hip)
//   k_xforc_slab.h   as the row-windowed kernels k_xf_*_win of the banded slab xforc: rows j0 .. j0 + gridDim.y - 1
//                    (compiled in k_xforc_slab.hip)
//
// An include rather than a __device__ function per kernel: with the functions qgcm_hip.hip no longer compiled to the
// device code it had (`make asm`, DESIGN 3.8: five of the k_xf_* kernels were scheduled differently); the included text
// preprocesses to the parent's token for token.
#pragma once
#include "qgcm_dev.h"

#define XF_NT 256
// the box average of ndxr above this is k_xf_wekpa_stage's (k_xf_wekpa_stage.h)
#define XF_WEKPA_STAGE_ABOVE 64

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


// cells a workgroup of k_xf_fine walks (k_xforc_rows.inc)
#define XF_CX 8
static_assert(XF_CX * 32 == XF_NT, "one thread gathers one of the 32 neighbourhood values of one cell");
