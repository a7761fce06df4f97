// k_tend_body.inc - the body of the tendency kernel (see k_tend.h), included into k_tend (ZM = 0) and k_tend_z (the
// zero-field variants).  Textual inclusion, not a device function: a by-value kernel argument that travels through a
// function parameter loses its address space (k_thomas_solve.inc), and k_tend is to compile to what it compiled to.
// The including kernel provides: template parameters NL, CYC, WTQ, AVG; the compile-time mask ZM (bit 0: entoc, bit 1:
// ddynoc is all zero: neither loaded nor given a prefetch register); QG_TEND_ARGS; the kernel arguments P, S, F.
  QG_STAMP(3, 10);
#ifndef TEND_EXPERIMENT // (tile-shape A/B builds without the mixed layer: profiles/r4_tend_shapes_socn5.log)
  static_assert(TEND_NT == OML_NT, "oml_final_block runs in workgroup 0 of this kernel");
#endif
  constexpr int TX = WTQ ? TEND_TX : TEND_TX_WIDE, TY = TEND_TY;
  static_assert(TEND_NT % TX == 0 && TY % (TEND_NT / TX) == 0, "whole rows of threads, whole rows per thread");
  constexpr int W3 = TX + 6, H3 = TY + 6; // pom tile, halo 3
  constexpr int W2 = TX + 4, H2 = TY + 4; // d2 tile, halo 2
  constexpr int W1 = TX + 2, H1 = TY + 2; // d4 / po / qo tiles, halo 1
  constexpr int N3 = (H3 * W3 + TEND_NT - 1) / TEND_NT; // staged elements per thread
  constexpr int N1 = (H1 * W1 + TEND_NT - 1) / TEND_NT;
  __shared__ double sp[H3 * W3];
  __shared__ double sd2[H2 * W2];
  // Del^4 tile: lives in the pom tile's storage (dead once Del^2 is formed; refilled only after the layer's
  // last barrier), which keeps the workgroup at 4 x 30 KB (TY = 8) resp. 3 x 51 KB (TY = 20) per CU
  double *sd4 = sp;
  static_assert(H1 * W1 <= H3 * W3, "Del^4 tile must fit into the pom tile");
  __shared__ double spo[H1 * W1];
  __shared__ double sqo[H1 * W1];

  // nx .. jhi (slab view: global row = local + joff), the row window and `side` are leading scalar arguments, preloaded
  // into SGPRs (QG_TEND_ARGS, qgcm_dev.h): the tile mapping and the staging offsets below wait for no scalar load
  const double *po0 = P.po, *qo0 = P.qo; // (requested here: they arrive while the offsets are formed)
  const long fs = P.g.fstride;
  const int tid = threadIdx.x;
  // ---- XCD-aware tile numbering ------------------------------------------
  // Box grids have nx = 64*g + 1 columns and (whole basin) 8*h + 1 rows: the last column and the last
  // row are walls whose update is point-wise (no stencil), so they are peeled off into a few "edge"
  // workgroups instead of a whole extra column / row of nearly empty tiles (tend_edge below).
  QgGeom gt; // what tend_tiling reads
  gt.nx = nx; gt.jlo = jlo; gt.jhi = jhi; gt.joff = joff; gt.nyg = nyg;
  const TendTiling T = tend_tiling<CYC, TX>(gt);
  const int gx = T.gx;
  const int ntiles = gx * (trows ? trows : T.gy); // (a window of the tile rows, or all of them)
  const int per_xcd = (ntiles + 7) / 8;
  if ((side & 1) && blockIdx.x == 0) {
    // mixed layer on, inside qgcm_hip_steps: the last reduction of `oml` (xon(1), enisoc(1) / eninoc(1), monitors) is
    // done here instead of in a one-workgroup launch; xon must be final before dpioc is stepped below
    __shared__ double redf[20];
    oml_final_block(F, redf, tid);
  }
  if (!CYC && (side & 2) && blockIdx.x == 0 && tid == 0) constr_dpi_update<NL>(P.sc, P.tdto, P.gpoc); // see QgTendParams
  if ((int)blockIdx.x >= 8 * per_xcd) {
    // cyclic / atmosphere: the boundary line sums for the momentum constraints (k_cyclic.h); box: the wall edges
    if (CYC) cyc_bsums_block(S, (int)blockIdx.x - 8 * per_xcd);
    else tend_edge<NL, AVG, ZM>(P, T, (int)blockIdx.x - 8 * per_xcd);
    return;
  }
  const int tile = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (tile >= ntiles) return;
  QG_STAMP(3, 0);
  const int i0 = (tile % gx) * TX + 1; // first global i of the tile (1-based)
  const int trow = trows ? trow0 + (tile / gx) * tstride : tile / gx;
  const int j0 = trow * TY + jlo; // first local row of the tile
  const int tx = tid % TX;
  const int ty0 = tid / TX; // 0..3
  constexpr int RPT = TY / (TEND_NT / TX); // rows per thread
  const double bcf = P.bcfaco, dxom2 = P.dxom2;

  // ---- global offsets of the elements this thread stages (same for every layer), computed ONCE: 32-bit element
  // offsets (the host checks ldx*ny*nl < 2^31) clamped to 0 where the element lies outside the array, plus a
  // validity bit. Every staging load is then unconditional: a "load or zero" conditional makes hipcc branch around
  // each load (exec-mask save / restore, s_cbranch_execz: ~560 of the kernel's 1900 instructions were that
  // bookkeeping, and the kernel is instruction-issue bound). Elements outside the array receive element 0 of the
  // field - a finite value that no point inside the domain ever reads.
  int o3[N3], o1[N1];
  bool v3[N3], v1[N1];
#pragma unroll
  for (int e = 0; e < N3; ++e) {
    int idx = tid + e * TEND_NT;
    int lx = idx % W3, ly = idx / W3;
    int gi = i0 - 3 + lx, gj = j0 - 3 + ly;
    v3[e] = idx < H3 * W3 && gj >= 1 && gj <= ny && (CYC ? (gi >= -2 && gi <= nx + 3) : (gi >= 1 && gi <= nx));
    o3[e] = v3[e] ? (gj - 1) * ldx + (tend_wrap<CYC>(gi, nxt) - 1) : 0;
  }
#pragma unroll
  for (int e = 0; e < N1; ++e) {
    int idx = tid + e * TEND_NT;
    int lx = idx % W1, ly = idx / W1;
    int gi = i0 - 1 + lx, gj = j0 - 1 + ly;
    v1[e] = idx < H1 * W1 && gj >= 1 && gj <= ny && (CYC ? (gi >= 0 && gi <= nx + 1) : (gi >= 1 && gi <= nx));
    o1[e] = v1[e] ? (gj - 1) * ldx + (tend_wrap<CYC>(gi, nxt) - 1) : 0;
  }
  double r3[N3], rp[N1], rq[N1];
  QG_STAMP(3, 11);
#pragma unroll
  for (int e = 0; e < N3; ++e) r3[e] = pom[o3[e]];
#pragma unroll
  for (int e = 0; e < N1; ++e) {
    rp[e] = po0[o1[e]];
    rq[e] = qo0[o1[e]];
  }
  // ---- the Del^2 / Del^4 passes of this thread (elements tid, tid + 256, ... of the halo-2 / halo-1 region): the LDS
  // read base, the position of the ONE inner neighbour the wall rule uses (N of a S-wall point, ...) and whether the
  // point is a wall point do not depend on the layer - computed once.  Points outside the domain are computed from
  // whatever the (clamped) loads delivered: no point inside the domain ever reads them (interior points have all five
  // neighbours inside, wall points read their inner neighbour only), so they need neither a predicate nor a select.
  constexpr int N2 = (H2 * W2 + TEND_NT - 1) / TEND_NT;
  int b2[N2], b4[N1], i2[N2], i4[N1];
  bool w2[N2], w4[N1];
#pragma unroll
  for (int e = 0; e < N2; ++e) {
    const int idx = tid + e * TEND_NT;
    const int lx = idx % W2, ly = idx / W2;
    const int gi = i0 - 2 + lx, gj = j0 - 2 + ly;
    b2[e] = (idx < H2 * W2) ? (ly + 1) * W3 + (lx + 1) : W3 + 1; // clamped: the extra pass reads valid LDS, stores nothing
    const bool wS = (gj + joff == 1), wN = (gj + joff == nyg), wW = (!CYC && gi == 1), wE = (!CYC && gi == nx);
    w2[e] = wS || wN || wW || wE;
    i2[e] = b2[e] + (wS ? W3 : (wN ? -W3 : (wW ? 1 : -1)));
  }
#pragma unroll
  for (int e = 0; e < N1; ++e) {
    const int idx = tid + e * TEND_NT;
    const int lx = idx % W1, ly = idx / W1;
    const int gi = i0 - 1 + lx, gj = j0 - 1 + ly;
    b4[e] = (idx < H1 * W1) ? (ly + 1) * W2 + (lx + 1) : W2 + 1;
    const bool wS = (gj + joff == 1), wN = (gj + joff == nyg), wW = (!CYC && gi == 1), wE = (!CYC && gi == nx);
    w4[e] = wS || wN || wW || wE;
    i4[e] = b4[e] + (wS ? W2 : (wN ? -W2 : (wW ? 1 : -1)));
  }
  // ---- epilogue operands of this thread's own points: requested while the LAST layer is computed (the
  // registers of the layer prefetch are free by then); the old qo of the wall rows is read in the epilogue
  constexpr bool ENT = !(ZM & 1), DDY = !(ZM & 2); // the field is read
  double e_qm[NL][RPT], e_wek[RPT], e_ent[ENT ? RPT : 1], e_ddy[DDY ? RPT : 1];
  double e_qo[AVG ? NL : 1][RPT]; // AVG: this step's qo of the thread's own points

  double dq[NL][RPT];
  double d2bot[RPT];

#pragma unroll
  for (int k = 0; k < NL; ++k) {
    // ---- registers -> LDS tiles of layer k --------------------------------
#pragma unroll
    for (int e = 0; e < N3; ++e) {
      int idx = tid + e * TEND_NT;
      if (idx < H3 * W3) sp[idx] = r3[e];
    }
#pragma unroll
    for (int e = 0; e < N1; ++e) {
      int idx = tid + e * TEND_NT;
      if (idx < H1 * W1) {
        spo[idx] = rp[e];
        sqo[idx] = rq[e];
      }
    }
    __syncthreads();
    QG_STAMP(3, 1 + 2 * k);
    // ---- issue the loads of layer k+1 (they fly while layer k is computed)
    if (k + 1 < NL) {
      const double *pomk = pom + fs * (k + 1);
      const double *po = po0 + fs * (k + 1);
      const double *qo = qo0 + fs * (k + 1);
#pragma unroll
      for (int e = 0; e < N3; ++e) r3[e] = pomk[o3[e]];
#pragma unroll
      for (int e = 0; e < N1; ++e) {
        rp[e] = po[o1[e]];
        rq[e] = qo[o1[e]];
      }
    } else {
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        int ly = ty0 + r * (TEND_NT / TX);
        int gi = i0 + tx, gj = j0 + ly;
        bool in = gi <= T.imax && gj <= T.jmax;
        const int o = in ? (gj - 1) * ldx + (gi - 1) : 0; // clamped: unconditional loads, values unused when !in
        e_wek[r] = P.wekpo[o];
        if (ENT) e_ent[ENT ? r : 0] = P.entoc[o];
        if (DDY) e_ddy[DDY ? r : 0] = P.ddynoc[o];
#pragma unroll
        for (int kk = 0; kk < NL; ++kk) e_qm[kk][r] = P.qnew[fs * kk + o];
        if (AVG) {
#pragma unroll
          for (int kk = 0; kk < NL; ++kk) e_qo[kk][r] = P.qo[fs * kk + o];
        }
      }
    }
    // ---- Del^2(pom) on the halo-2 region (qgosubs.F:94-127) ----------
#pragma unroll
    for (int e = 0; e < N2; ++e) {
      const int idx = tid + e * TEND_NT;
      const double *c = &sp[b2[e]];
      // branch-free: the wall rule picks ONE inner neighbour (N, S, E or W of a wall point), the interior rule is
      // evaluated alongside and the result selected - qg_ref_expr.h's expressions, no exec-mask bookkeeping
      const double cS = c[-W3], cW = c[-1], c0 = c[0], cE = c[1], cN = c[W3];
      const double vw = QG_WALL_RULE(bcf, sp[i2[e]], c0);
      const double vi = QG_FIVE_POINT(cS, cW, cE, cN, c0) * dxom2;
      if (idx < H2 * W2) sd2[idx] = w2[e] ? vw : vi;
    }
    __syncthreads();
    // ---- Del^4 on the halo-1 region (qgosubs.F:310-341) ---------------
#pragma unroll
    for (int e = 0; e < N1; ++e) {
      const int idx = tid + e * TEND_NT;
      const double *c = &sd2[b4[e]];
      const double cS = c[-W2], cW = c[-1], c0 = c[0], cE = c[1], cN = c[W2];
      const double vw = QG_WALL_RULE(bcf, sd2[i4[e]], c0);
      const double vi = dxom2 * QG_FIVE_POINT(cS, cW, cE, cN, c0);
      if (idx < H1 * W1) sd4[idx] = w4[e] ? vw : vi;
    }
    __syncthreads();
    // ---- Del^6 + Jacobian at the tile's own points (qgosubs.F:349-399)
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      int ly = ty0 + r * (TEND_NT / TX);
      int gi = i0 + tx, gj = j0 + ly;
      double val = 0.0;
      bool interior = (gj <= jhi && gj + joff >= 2 && gj + joff <= nyg - 1) && (CYC ? (gi >= 1 && gi <= nx) : (gi >= 2 && gi <= nx - 1));
      if (interior) {
        const double *d4 = &sd4[(ly + 1) * W1 + (tx + 1)];
        const double *p = &spo[(ly + 1) * W1 + (tx + 1)];
        const double *q = &sqo[(ly + 1) * W1 + (tx + 1)];
        double d6p = dxom2 * QG_FIVE_POINT(d4[-W1], d4[-1], d4[1], d4[W1], d4[0]);
        double diffus = P.ah2fac[k] * d4[0] - P.ah4fac[k] * d6p;
        // (the halves of qg_ref_expr.h's Jacobian chain to the one left-to-right sum: the same bits.  The compiler barrier
        //  between them exists in the wide-tile variants only: there the LDS reads of all twelve terms in flight at once left
        //  k_tend_z<2, true, false, false, 3> with 84 VGPRs against its twin's 82; with it the wide variants take 72 / 86 / 90
        //  VGPRs for 2 / 3 / 4 layers instead of 82 / 96 / 100.  k_tend and the 16-wide variants compile as without it.)
        double jac = QG_JAC_HEAD(q[-W1], q[-1], q[1], q[W1], p[-W1], p[-1], p[1], p[W1],
                                 p[-W1 - 1], p[-W1 + 1], p[W1 - 1], p[W1 + 1]);
        if (ZM && !WTQ) asm volatile("" ::: "memory");
        jac = QG_JAC_TAIL(jac, p[-W1], p[-1], p[1], p[W1], q[-W1 - 1], q[-W1 + 1], q[W1 - 1], q[W1 + 1]);
        val = P.adfaco * jac + diffus;
      }
      dq[k][r] = val;
      if (k == NL - 1) d2bot[r] = sd2[(ly + 2) * W2 + (tx + 2)];
    }
    QG_STAMP(3, 2 + 2 * k);
    if (k + 1 < NL) __syncthreads();
  }

  // ---- forcing, bottom drag, leapfrog, projection ----------------------
  if (WTQ) {
    // (every lane goes through: the stores are pairs of neighbouring lanes; points outside the tile's part of the
    //  domain compute on clamped operands and store nothing)
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      int ly = ty0 + r * (TEND_NT / TX);
      const int gi0 = i0 + tx, gj0 = j0 + ly;
      const bool valid = gi0 <= T.imax && gj0 <= T.jmax;
      const int gi = valid ? gi0 : (gi0 <= T.imax ? gi0 : T.imax), gj = gj0 <= T.jmax ? gj0 : T.jmax;
      double dqp[NL], qmp[NL], qop[NL];
      const bool wallrow = (gj + joff == 1 || gj + joff == nyg);
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        dqp[k] = dq[k][r];
        qmp[k] = e_qm[k][r];
        qop[k] = AVG ? e_qo[AVG ? k : 0][r] : (wallrow ? P.qo[fs * k + (long)(gj - 1) * ldx + (gi - 1)] : 0.0);
      }
      // (a field the host knows to be all zero enters as a literal 0.0: the same expressions, the same bits)
      tend_point<NL, CYC, true, AVG>(P, gi0, gj, dqp, d2bot[r], qmp, qop, e_wek[r], ENT ? e_ent[ENT ? r : 0] : 0.0,
                                     DDY ? e_ddy[DDY ? r : 0] : 0.0, valid);
    }
  } else {
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      int ly = ty0 + r * (TEND_NT / TX);
      int gi = i0 + tx, gj = j0 + ly;
      if (gi > T.imax || gj > T.jmax) continue;
      double dqp[NL], qmp[NL], qop[NL];
      const bool wallrow = (gj + joff == 1 || gj + joff == nyg);
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        dqp[k] = dq[k][r];
        qmp[k] = e_qm[k][r];
        qop[k] = AVG ? e_qo[AVG ? k : 0][r] : (wallrow ? P.qo[fs * k + (long)(gj - 1) * ldx + (gi - 1)] : 0.0);
      }
      tend_point<NL, CYC, false, AVG>(P, gi, gj, dqp, d2bot[r], qmp, qop, e_wek[r], ENT ? e_ent[ENT ? r : 0] : 0.0,
                                      DDY ? e_ddy[DDY ? r : 0] : 0.0);
    }
  }
  QG_STAMP(3, 7);
  QG_STAMP_DRAIN();
  QG_STAMP(3, 8);
