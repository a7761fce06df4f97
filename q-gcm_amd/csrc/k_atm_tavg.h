// k_atm_tavg.h - the atmosphere's time averages and periodic dump on the device.
//
// Two products of the reference that otherwise need pa, qa on the host:
//   * tavatm / tavout, atmosphere half (src/timavge.F:278-421, 715-801): sums of the wind stress, wekta, fnetat, ast,
//     pa, qa and of the atmospheric mixed layer's C-grid advection terms uufa .. vtvfa; tavout scales them by
//     rnsat = 1/nsumat (0 when nsumat = 0) and derives the eddy fluxes uptpat / vptpat.
//   * atnc_out (src/nc_subs.F:1077-1326): ast, pa, qa, wekta, ha, tauxa, tauya, hmixa at the subsampled points.
// Everything is elementwise with the reference's expressions in the reference's order (built with -ffp-contract=off):
// bitwise the reference's numbers.  No atomics, no scratch.
//
// The sums use the ocean's layout (k_tavg.h) under the atmosphere's names, so that k_tav_mean<NL> serves tavout
// unchanged: TAV_TX, TAV_TY txatav, tyatav | TAV_WP unused | TAV_WT, TAV_FM, TAV_SST wtatav, fmatav, astav |
// patav (nla) | qatav (nla) | uufa, tufa, utufa | vvfa, tvfa, vtvfa; the means append uptpat, vptpat.  QgTavParams
// carries po = pa, qo = qa, taux / tauy = tauxa / tauya, wekto = wekta, sst = ast, fnet = fnetat, uvgfac = rdxaf0.
// What differs from the cyclic ocean's tavocn (k_tav_accum) and is honoured here:
//   - the Ekman terms' signs: uuf = -rdxaf0*dpa - rhf0hm*(tauya+tauya), vvf = rdxaf0*dpa + rhf0hm*(tauxa+tauxa);
//   - column nxpa of the zonal terms is computed from pa(nxpa,.) and tauya(nxpa,.) themselves (no copy of column 1),
//     with tuf(1) = tuf(nxpa) = 0.5*(ast(1,j) + ast(nxta,j));
//   - p rows 1 and nypa: vvf = vtvf = 0, tvf = ast(i,1) resp. ast(i,nypa-1) (no sb_hflux / nb_hflux branch);
//   - no Ekman-pumping sum (TAV_WP stays zero).
//
//   k_tavat_accum   one tavatm contribution over the whole domain
//   k_atnc_sample   atnc_out's subsampled fields, one plane per grid z (ha with the reference's division)
#pragma once
#include "qgcm_dev.h"
#include "k_tavg.h"

// One thread per p point (i, j): the p-grid sums and vvfa .. vtvfa (i <= nxta) of p row j; for T rows (j <= nyta)
// also the T-grid sums (i <= nxta) and uufa .. utufa of T row j.
template <int NL>
__global__ __launch_bounds__(TAV_NT) void k_tavat_accum(const QgTavParams P) {
  const int nx = P.g.nx, nxt = P.g.nxt, ldx = P.g.ldx, ldt = P.ldt, ny = P.g.ny;
  const long fs = P.g.fstride;
  const int i = blockIdx.x * TAV_NT + threadIdx.x + 1; // 1-based
  const int j = blockIdx.y + 1;
  if (i > nx || j > ny) return;
  const long ip = (long)(i - 1) + (long)ldx * (j - 1);
  const double *pa = P.po, *ast = P.sst, *tx = P.taux, *ty = P.tauy;
  const double rdxaf0 = P.uvgfac, rh = P.rhf0hm;
  double *S = P.sum;
  // wind stress (p grid)
  S[TAV_TX * fs + ip] = S[TAV_TX * fs + ip] + tx[ip];
  S[TAV_TY * fs + ip] = S[TAV_TY * fs + ip] + ty[ip];
  const long it = (long)(i - 1) + (long)ldt * (j - 1); // T point (i, j)
  const int u = TAV_UU(NL);
  // meridional advection at p row j (T columns i = 1..nxta); rows 1 and nypa: the zonal boundaries
  if (i <= nxt) {
    double vvf, tvf, vtvf;
    if (j == 1) {
      vvf = 0.0;
      tvf = ast[it];
      vtvf = 0.0;
    } else if (j == ny) {
      vvf = 0.0;
      tvf = ast[it - ldt]; // ast(i, nypa-1)
      vtvf = 0.0;
    } else {
      vvf = rdxaf0 * (pa[ip + 1] - pa[ip]) + rh * (tx[ip + 1] + tx[ip]);
      tvf = 0.5 * (ast[it] + ast[it - ldt]);
      vtvf = vvf * tvf;
    }
    S[(u + 3) * fs + ip] = S[(u + 3) * fs + ip] + vvf;
    S[(u + 4) * fs + ip] = S[(u + 4) * fs + ip] + tvf;
    S[(u + 5) * fs + ip] = S[(u + 5) * fs + ip] + vtvf;
  }
  if (j < ny) {
    // T-grid fields of T row j
    if (i <= nxt) {
      S[TAV_WT * fs + ip] = S[TAV_WT * fs + ip] + P.wekto[it];
      S[TAV_FM * fs + ip] = S[TAV_FM * fs + ip] + P.fnet[it];
      S[TAV_SST * fs + ip] = S[TAV_SST * fs + ip] + ast[it];
    }
    // zonal advection at T row j (p columns i = 1..nxpa): tuf(1) and tuf(nxpa) both 0.5*(ast(1,j) + ast(nxta,j))
    const long row = (long)ldt * (j - 1);
    const double tuf = (i == 1 || i == nx) ? 0.5 * (ast[row] + ast[row + nxt - 1]) : 0.5 * (ast[row + i - 1] + ast[row + i - 2]);
    const double uuf = -(rdxaf0 * (pa[ip + ldx] - pa[ip])) - rh * (ty[ip + ldx] + ty[ip]);
    S[u * fs + ip] = S[u * fs + ip] + uuf;
    S[(u + 1) * fs + ip] = S[(u + 1) * fs + ip] + tuf;
    S[(u + 2) * fs + ip] = S[(u + 2) * fs + ip] + uuf * tuf;
  }
  // pa and qa in the reference's last loop (the order of independent sums does not matter)
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    S[(TAV_P0 + k) * fs + ip] = S[(TAV_P0 + k) * fs + ip] + pa[k * fs + ip];
    S[(TAV_P0 + NL + k) * fs + ip] = S[(TAV_P0 + NL + k) * fs + ip] + P.qo[k * fs + ip];
  }
}

// atnc_out's planes: ast | pa (nla) | qa (nla) | wekta | ha (nla-1) | tauxa, tauya | hmixa, the selected ones
#define ATNC_MAXP (4 * QG_MAXL)
struct QgAtncParams {
  const double *src[ATNC_MAXP], *src2[ATNC_MAXP]; // src2: pa(k+1) of an ha plane, else nullptr
  double gp[ATNC_MAXP];                           // gpat(k) of an ha plane
  long off[ATNC_MAXP];                            // first output element of the plane
  int ld[ATNC_MAXP], ni[ATNC_MAXP], nj[ATNC_MAXP];
  int nska;
  double *out;
};

// element (i, j) of plane z: the point (1 + i*nska, 1 + j*nska), i fastest, as the reference fills wrk
__global__ __launch_bounds__(256) void k_atnc_sample(const QgAtncParams P) {
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, z = blockIdx.z;
  if (i >= P.ni[z] || j >= P.nj[z]) return;
  const long o = (long)j * P.nska * P.ld[z] + (long)i * P.nska;
  // ha = ( pa(k) - pa(k+1) )/gpat(k)   (src/nc_subs.F:1257-1259)
  const double v = P.src2[z] ? (P.src[z][o] - P.src2[z][o]) / P.gp[z] : P.src[z][o];
  P.out[P.off[z] + (long)j * P.ni[z] + i] = v;
}
