// k_thomas_corr.inc - the body of the correction pass (see k_thomas.h), included into k_thomas_corr (this handle is slab
// P.rank of P.nranks), k_thomas_corr_seg (segment `rank` of the P.nranks segments of one column) and k_thomas_corr_slab
// (k_thomas_slab.h: one segment of slab P.rank); textual inclusion for the reason given in k_thomas_solve.inc.  The
// including kernel provides: the kernel argument P; T (its QgThomasCorr, or a segment's); rank, jr0, jr1 (the rows
// corrected); slice (of THC_UNR * STEP rows); owner: this workgroup publishes the basin-wide ksum / ybnd;
// and, where the rows corrected are not all of `rank`, the macro THC_INFLOWS(u, v), which turns the inflows composed
// for `rank` into theirs (a macro, not a callable: an empty lambda reordered a few instructions of the two kernels that
// have nothing to turn, and they are to compile to what they compiled to).
  // 256 threads: four workgroups share a CU (the pass is all memory latency).  Every thread first requests its first
  // rows and table entries, then the workgroup fetches all ranks' summaries of the block's 16 wavenumbers into LDS in
  // one round trip - the two latencies overlap instead of adding - and 16 lanes run the two short chains of
  // multiply-adds over the ranks.  (Measured, NAtl 1 km, 600-row slabs: 1024-thread workgroups
  // composing with one wave scan per wavenumber 20.8 us; 256 threads, four scans per wave one after the other: 24.5 us.)
  __shared__ double sU[TH_KW], sV[TH_KW];
  extern __shared__ double sG[]; // dynamic: nranks x (THC_PER doubles of summaries and constants + TH_KW inflows)
  const int tid = threadIdx.x;
  const int bx = blockIdx.x, m = blockIdx.y + P.layer0;
  const int ldw = P.g.ldw;
  const double ft = P.ftnorm;
  const int tb = m * P.nblk + bx;
  const int np = T.np[tb], nq = T.nq[tb];
  const int nr = jr1 - jr0 + 1;
  const int kp = tid & 7, c = tid >> 3; // pair of wavenumbers 2 kp, 2 kp + 1 of the block; rows c, c + 32, ...
  constexpr int STEP = THC_NT / 8;
  const bool pair_ok = bx * TH_KW + 2 * kp < P.g.nk; // (the second of a pair may be the row's padding column: ldw > nk)
  double *wb = P.wrk + P.g.wstride * m + (long)(jr0 - 1) * ldw + bx * TH_KW + 2 * kp;
  const double *pt = T.ptab + (long)T.poff[tb] * TH_KW + 2 * kp;
  const double *qt = T.qtab + (long)T.qoff[tb] * TH_KW + 2 * kp;
  const int q0 = nr - nq; // first row the upper inflow reaches (table row r - q0)
  // the rows to correct: [0, np) and [max(np, q0), nr), as one index space of n1 + n2 rows
  const int n1 = np, s2 = np > q0 ? np : q0, ntot = n1 + (nr - s2);
  double2 w[THC_UNR], a[THC_UNR], b[THC_UNR];
  auto row_of = [&](int x) { return x < n1 ? x : s2 + (x - n1); };
  auto request = [&](int x0) {
#pragma unroll
    for (int i = 0; i < THC_UNR; ++i) {
      const int x = x0 + i * STEP;
      const int r = row_of(x < ntot ? x : ntot - 1); // clamped: unconditional loads
      w[i] = *reinterpret_cast<const double2 *>(wb + (long)r * ldw);
      a[i] = double2{0.0, 0.0};
      b[i] = double2{0.0, 0.0};
      if (r < np) a[i] = *reinterpret_cast<const double2 *>(pt + (long)r * TH_KW);
      if (r >= q0 && nq > 0) b[i] = *reinterpret_cast<const double2 *>(qt + (long)(r - q0) * TH_KW);
    }
  };
  // slice (blockIdx.z of k_thomas_corr): slice of THC_UNR * STEP = 128 of those rows (one trip of the loop below per workgroup: the blocks of
  // the lowest wavenumbers, whose responses reach through the whole slab, otherwise run 5 trips = 5 memory round trips
  // one after the other while everybody else has long finished - measured 22.7 us per 600-row slab of NAtl 1 km)
  const int xa = slice * (THC_UNR * STEP), xb0 = xa + THC_UNR * STEP, xb = xb0 < ntot ? xb0 : ntot;
  if (slice > 0 && xa >= ntot) return; // (uniform; slice 0 always composes: it owns ksum / ybnd)
  const bool work = xa < ntot && pair_ok;
  if (work) request(xa + c);
  // every rank's summaries (Cf, Cb, S0) and constants (D, E, SP, SQ) of the block's 16 wavenumbers: 48 + 64 contiguous
  // doubles per rank, fetched by the whole workgroup in one round trip
  {
    const long mk0 = TH_MSG * ((long)m * ldw + bx * TH_KW), ck0 = TH_CST * ((long)m * ldw + bx * TH_KW);
    const long cstride = (long)TH_CST * P.g.nl * ldw;
    // (four loads in flight per trip: a rolled loop waits for every load before it requests the next - with eight ranks
    //  that was four memory round trips one after the other in every workgroup's latency chain, now one)
    const int total = P.nranks * THC_PER;
    for (int it0 = tid; it0 < total; it0 += 4 * THC_NT) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int it = it0 + u * THC_NT, itc = it < total ? it : 0;
        const int sr = itc / THC_PER, jj = itc - sr * THC_PER;
        v[u] = jj < TH_MSG * TH_KW ? P.gath[(long)sr * P.gath_stride + mk0 + jj] : P.cgath[(long)sr * cstride + ck0 + (jj - TH_MSG * TH_KW)];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int it = it0 + u * THC_NT;
        if (it < total) {
          const int sr = it / THC_PER, jj = it - sr * THC_PER;
          sG[sr * THC_LDS + jj] = v[u];
        }
      }
    }
  }
  __syncthreads();
  if (tid < TH_KW) {
    // lane = wavenumber kq of the block; ranks s = 0 .. nranks-1 in turn (operands in LDS: two short chains)
    const int kq = bx * TH_KW + tid;
    const double *gk = sG + TH_MSG * tid, *ck = sG + TH_MSG * TH_KW + TH_CST * tid;
    // forward chain: value leaving rank s = Cf_s + D_s * (value entering rank s), nothing enters rank 0
    double u = 0.0, mine_u = 0.0, vlast = 0.0;
    for (int sr = 0; sr < P.nranks; ++sr) {
      sG[sr * THC_LDS + THC_PER + tid] = u;
      if (sr == rank) mine_u = u;
      u = __builtin_fma(ck[sr * THC_LDS], u, gk[sr * THC_LDS]);
      vlast = u;
    }
    // backward chain, last rank first: value leaving rank s downwards = Cb_s + E_s*uin_s + D_s * (value entering from above)
    double v = 0.0, mine_v = 0.0, term = 0.0, vfirst = 0.0;
    for (int sr = P.nranks - 1; sr >= 0; --sr) {
      const double *gs = gk + sr * THC_LDS, *gc = ck + sr * THC_LDS;
      const double us = sG[sr * THC_LDS + THC_PER + tid];
      if (sr == rank) mine_v = v;
      term += gs[2] + us * gc[2] + v * gc[3]; // column sum of rank s: S0 + uin*SP + vin*SQ
      v = __builtin_fma(gc[0], v, gs[1] + gc[1] * us);
      vfirst = v;
    }
#ifdef THC_INFLOWS
    THC_INFLOWS(mine_u, mine_v);
#endif
    sU[tid] = ft * mine_u;
    sV[tid] = ft * mine_v;
    if (kq < P.g.nk && owner) P.ksum[(long)m * ldw + kq] = ft * term;
    if (P.ybnd && kq == 0 && owner) {
      // cyclic constraints: the zonal-mean solution next to the two zonal boundaries, on every rank, from the
      // summaries: the value leaving rank 0 downwards is the solution at its first row (global row 2); the forward
      // value leaving the last rank is the solution at its last row (global row nyg-1: nothing enters from above)
      P.ybnd[2 * m] = ft * vfirst;
      P.ybnd[2 * m + 1] = ft * vlast;
    }
  }
  if (xa >= ntot) return; // (uniform: no barrier is skipped by part of the workgroup)
  __syncthreads();
  if (!pair_ok) return;
  const double u0 = sU[2 * kp], u1 = sU[2 * kp + 1], v0 = sV[2 * kp], v1 = sV[2 * kp + 1];
  {
    const int x0 = xa + c;
#pragma unroll
    for (int i = 0; i < THC_UNR; ++i) {
      const int x = x0 + i * STEP;
      if (x < xb) {
        const double xx = __builtin_fma(v0, b[i].x, __builtin_fma(u0, a[i].x, w[i].x));
        const double yy = __builtin_fma(v1, b[i].y, __builtin_fma(u1, a[i].y, w[i].y));
        qg_store16_wt(wb + (long)row_of(x) * ldw, xx, yy);
      }
    }
  }
