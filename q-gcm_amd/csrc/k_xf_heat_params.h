// k_xf_heat_params.h - what the kernels of xforc's heat half read (k_xforc.h: k_xf_heat_oc, k_xf_heat_atm,
// k_xf_heat_final; k_xf_heat_sst.h: k_xf_heat_sst, compiled in a translation unit of its own).
#pragma once

struct QgXfHeatParams {
  int nxta, nyta, nxto, nyto, ndxr, nx1, ny1, nxaooc, nyaooc;
  int ldta, lda, ldto;             // pitches: atmosphere T / p grid, ocean T grid
  long fstride;                    // doubles between two layers of pam
  const double *astm, *hmm, *pam, *dtop; // atmosphere: lagged levels (T grid), lagged pressure, topography (or nullptr)
  const double *sstm;              // ocean: lagged mixed-layer temperature
  const double *fsa, *fso;         // fsprim tables (nyta), (nyto)
  const int *ix, *iy;              // iam, iap (2, nxto); jam, jap (2, nyto): 1-based
  const double *wx, *wy;           // wmx, wpx (2, nxto); wmy, wpy (2, nyto)
  double *fnetoc, *fnetat;
  double *cell;                    // (nxaooc, nyaooc) sums above the ocean
  double *part;                    // (3, ncell) arocsm, slhfsm, oradsm per cell, then (nblkL) arlasm per workgroup of k_xf_heat_atm
  double *scal;                    // arlaav, slhfav, oradav, arocav
  int ncell, nblkL, natlan;
  double D0up, xlamda, Dmdown, Dmup, dmdu, ocfrac, fmafac, fmatop, hmafac, hmat, ocnorm;
};
