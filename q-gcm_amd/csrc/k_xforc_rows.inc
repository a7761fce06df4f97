// k_xforc_rows.inc - the text of the atmosphere-side kernels of xforc's momentum half, included once per set of kernels
// (k_xforc_rows.h says by whom and why).  The includer defines
//
//   XF_K(name)       the kernel's name                          k_xforc.h: name          k_xforc_slab.h: name##_win
//   XF_WIN_ARG       further kernel arguments                   (none)                   , const QgXfWin W
//   XF_J0            the row of blockIdx.y = 0                  1                        W.j0
//   XF_JUMAX         k_xf_atm: the last row that forms uekat    P.nyta                   W.jumax
//   XF_SOUTH/NORTH   k_xf_lines: form txisat / txinat           true                     (W.lines & 1) / (W.lines & 2)
//   XF_LINES_OC      k_xf_lines: the cyclic ocean's two sums    P.sco != nullptr         false
//   XF_WINDOWED      0 / 1 (k_xf_tauo has no windowed form: a slab's rows are its whole grid)
//
// Indices in comments are the reference's 1-based ones.

// grid: (ceil(nxpa/256), rows)
__global__ __launch_bounds__(XF_NT) void XF_K(k_xf_coarse)(const QgXfParams P XF_WIN_ARG) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + XF_J0;
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

// grid: (ceil(nxta/XF_CX), cell rows): one workgroup per XF_CX zonally adjacent coarse T cells (ic, jc).  A thread owns one
// fine point (ii, jj) of a cell, keeps that point's 16 (+16 next to a zonal boundary) weights in registers and walks
// the workgroup's cells with them, so a weight is fetched once per XF_CX cells; the cells' 16-point neighbourhoods of
// u1at / v1at sit in LDS (one wave-uniform read per term).  With one cell per workgroup the weight reads from L2 -
// 256 bytes per fine point against 16 stored - bound the kernel (profiles/xforc.log).
__global__ __launch_bounds__(XF_NT) void XF_K(k_xf_fine)(const QgXfParams P XF_WIN_ARG) {
  __shared__ double dat[XF_CX][32]; // per cell udat(1..16), vdat(1..16)
  const int ic0 = blockIdx.x * XF_CX + 1, jc = blockIdx.y + XF_J0, tid = threadIdx.x;
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

// grid: (ceil(nxpa/256), rows)
__global__ __launch_bounds__(XF_NT) void XF_K(k_xf_atm)(const QgXfParams P XF_WIN_ARG) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, ja = blockIdx.y + XF_J0;
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
  if (ja <= XF_JUMAX) { // uekat(nxpa, nyta): tauy along the meridional side; uekat(nxpa, ja) = uekat(1, ja)
    const int ic = (ia == P.nxpa) ? 1 : ia;
    const double *t = P.tyf + (long)(joff - 1) * ldf + (long)(ic - 1) * ndxr;
    double s = 0.5 * t[0];
    for (int j = 1; j < ndxr; ++j) s = s + t[(long)j * ldf];
    s = s + 0.5 * t[(long)ndxr * ldf];
    P.uekat[(long)(ja - 1) * P.lda + (ia - 1)] = -P.uvekfc * s;
  }
}

// grid: (ceil(nxta/256), rows)
__global__ __launch_bounds__(XF_NT) void XF_K(k_xf_wekta)(const QgXfParams P XF_WIN_ARG) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, ja = blockIdx.y + XF_J0;
  if (ia > P.nxta) return;
  const double *ue = P.uekat + (long)(ja - 1) * P.lda + (ia - 1);
  const double *ve = P.vekat + (long)(ja - 1) * P.ldta + (ia - 1);
  P.wekta[(long)(ja - 1) * P.ldta + (ia - 1)] = -P.hmrdxa * (ue[1] - ue[0] + ve[P.ldta] - ve[0]);
}

// grid: (ceil(nxtaor/256), fine T rows)
__global__ __launch_bounds__(XF_NT) void XF_K(k_xf_wektaor)(const QgXfParams P XF_WIN_ARG) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + XF_J0;
  if (i > P.nxtaor) return;
  const int ld = P.ldf;
  const long o = (long)(j - 1) * ld + (i - 1); // (i, j); (i+1, j) = o+1; (i, j+1) = o+ld
  const double *tx = P.txf, *ty = P.tyf;
  P.wf[(long)(j - 1) * P.ldtf + (i - 1)] =
      P.hxofac * (ty[o + 1] + ty[o + ld + 1] - (ty[o] + ty[o + ld]) + tx[o] + tx[o + 1] - (tx[o + ld] + tx[o + ld + 1]));
}

// grid: (ceil(nxpa/64), rows)
__global__ __launch_bounds__(64) void XF_K(k_xf_wekpa)(const QgXfParams P XF_WIN_ARG) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, ja = blockIdx.y + XF_J0;
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

#if !XF_WINDOWED
// grid: (ceil(nxpo/256), nypo)
__global__ __launch_bounds__(XF_NT) void k_xf_tauo(const QgXfParams P) {
  const int io = blockIdx.x * blockDim.x + threadIdx.x + 1, jo = blockIdx.y + 1;
  if (io > P.nxpo) return;
  const long f = (long)(P.jocoff + jo - 1) * P.ldf + (P.iocoff + io - 1), o = (long)(jo - 1) * P.ldo + (io - 1);
  P.tauxo[o] = P.raoro * P.txf[f];
  P.tauyo[o] = P.raoro * P.tyf[f];
}
#endif

// One workgroup of 256.  Sums 0, 1: the atmosphere's southern / northern line (fine tauxaor rows jsou, jnor; odd ndxr:
// the pairs with rows jsou+1, jnor-1); sums 2, 3: the cyclic ocean's (tauxo rows 1+2, nypo-1+nypo).  Trapezoid end
// weights.  Fixed order: thread-strided along the row, wave butterfly, waves left to right.  A sum that is not asked
// for (XF_SOUTH, XF_NORTH, XF_LINES_OC) reads no row and writes no scalar.
__global__ __launch_bounds__(XF_NT) void XF_K(k_xf_lines)(const QgXfParams P XF_WIN_ARG) {
  __shared__ double red[4][XF_NT / 64];
  const int tid = threadIdx.x, ndxr = P.ndxr;
  const int jsou = 1 + ndxr / 2, jnor = P.nypaor - ndxr / 2;
  const bool oc = XF_LINES_OC;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 1 + tid; i <= P.nxpaor; i += XF_NT) {
    const double w = (i == 1 || i == P.nxpaor) ? 0.5 : 1.0;
    const double *c = P.txf + (i - 1);
    double a = XF_SOUTH ? c[(long)(jsou - 1) * P.ldf] : 0.0, b = XF_NORTH ? c[(long)(jnor - 1) * P.ldf] : 0.0;
    if (P.ndxodd) {
      if (XF_SOUTH) a = a + c[(long)jsou * P.ldf];
      if (XF_NORTH) b = b + c[(long)(jnor - 2) * P.ldf];
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
    if (XF_SOUTH) P.sca->txisoc = fa * t[0];
    if (XF_NORTH) P.sca->txinoc = fa * t[1];
    if (oc) {
      P.sco->txisoc = 0.5 * P.dxo * t[2];
      P.sco->txinoc = 0.5 * P.dxo * t[3];
    }
  }
}
