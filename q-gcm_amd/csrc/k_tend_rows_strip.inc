// k_tend_rows_strip.inc - phase 1 of k_tend_rows (k_tend_rows.h) for ONE strip of a band: the text of the strip body,
// included twice, with TR_WALLS 1 (a strip within reach of a wall row or wall column) and 0 (every row j0-3 .. j0+B+2 and
// every lane's column lies inside the array, no lane is a wall column, the band is whole).  With TR_WALLS 0 the five-point
// operator is the interior sum alone and there are no row or column clamps, no cint / isW / isE and no partial-band break:
// at a point out of reach of the walls the selects of the wall body return exactly these values, so the bits are the same.
// In scope: the kernel's locals (pom, po0, qo0, fs, lds, lane, nx, ny, ldx, jr1, dxom2, R) and the strip loop's: `strip`,
// jb (the band's first row j0, as this strip sees it) and PE (the parameter block P, as this strip reads it) - see there.
{
  constexpr bool WALLS = TR_WALLS;
  const int i0 = strip * TR_SW + 1;          // first column the strip owns (odd)
  const int gi = i0 - TR_HL + lane;          // this lane's column
  // clamped: lanes outside the basin load finite values no point inside reads
  const int gc = WALLS ? (gi < 1 ? 1 : (gi > nx ? nx : gi)) : gi;
  const unsigned lcol = (unsigned)(gc - 1) * 8u;
  const bool lown = lane >= TR_HL && lane < TR_HL + TR_SW;
  const bool own = WALLS ? (lown && gi <= nx) : lown; // (gi >= 1 then)
  const bool cint = WALLS ? (gi >= 2 && gi <= nx - 1) : true;
  if (WALLS) {
    R.isW = gi == 1;
    R.isE = gi == nx;
  }
  // row offset inside a field layer; clamped within reach of the walls: rows outside the array are never used by a point inside
  auto rowoff = [&](int gj) {
    const int rj = WALLS ? (gj < 1 ? 1 : (gj > ny ? ny : gj)) : gj;
    return (unsigned)((rj - 1) * ldx) * 8u;
  };
  // gj: the row of c0, in a VGPR for the wall rule (tr_lap)
  auto lap = [&](double cS, double c0, double cN, int gj) {
    if constexpr (WALLS) return tr_lap(R, cS, c0, cN, gj + R.vz);
    else return tr_lap_interior(R.dxom2, cS, c0, cN);
  };

  double w[B + 6], pr[B + 2], qr[B + 2]; // pom rows jb-3 .. jb+B+2, po / qo rows jb-1 .. jb+B of the layer in flight
#pragma unroll
  for (int r = 0; r < B + 6; ++r) w[r] = tr_ld(pom, rowoff(jb - 3 + r) + lcol);
#pragma unroll
  for (int r = 0; r < B + 2; ++r) {
    pr[r] = tr_ld(po0, rowoff(jb - 1 + r) + lcol);
    qr[r] = tr_ld(qo0, rowoff(jb - 1 + r) + lcol);
  }
  double dq[NL][B], d2bot[B];
  double e_qm[NL][B], e_wek[B], e_ent[ENT ? B : 1], e_ddy[DDY ? B : 1];
  // yporel of the band's rows, on the SCALAR path (the table is written when the handle is set up, never during a step):
  // read as a per-row global load inside the epilogue it was a vector load of a wave-uniform value whose wait,
  // vmcnt(0), also waited for the acknowledgement of the row's write-through stores (k_tend_rows.h)
  double e_yp[B];
  // (TR_FENCE, TR_PIN: k_tend_rows.h - between the fences the order is the one written here)
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    // Del^2 of rows jb-2 .. jb+B+1
    double d2[B + 4], d4[B + 2];
#pragma unroll
    for (int r = 0; r < B + 4; ++r) {
      d2[r] = lap(w[r], w[r + 1], w[r + 2], jb - 2 + r);
      TR_PIN(d2[r]);
    }
    TR_FENCE();
    if (k + 1 < NL) {
      const double *pomk = pom + fs * (k + 1);
#pragma unroll
      for (int r = 0; r < B + 6; ++r) w[r] = tr_ld(pomk, rowoff(jb - 3 + r) + lcol);
    } else { // the operands of the point-wise epilogue
      const TrConstRow yprow = (TrConstRow)PE.yporel;
#pragma unroll
      for (int t = 0; t < B; ++t) e_yp[t] = yprow[(WALLS && jb + t > ny ? ny : jb + t) - 1]; // (a partial band: clamped, unused)
#pragma unroll
      for (int t = 0; t < B; ++t) {
        const unsigned o = rowoff(jb + t) + lcol;
        e_wek[t] = tr_ld(PE.wekpo, o);
        if (ENT) e_ent[ENT ? t : 0] = tr_ld(PE.entoc, o);
        if (DDY) e_ddy[DDY ? t : 0] = tr_ld(PE.ddynoc, o);
#pragma unroll
        for (int kk = 0; kk < NL; ++kk) e_qm[kk][t] = tr_ld(PE.qnew + fs * kk, o);
      }
    }
    TR_FENCE();
    // Del^4 of rows jb-1 .. jb+B
#pragma unroll
    for (int r = 0; r < B + 2; ++r) {
      d4[r] = lap(d2[r], d2[r + 1], d2[r + 2], jb - 1 + r);
      TR_PIN(d4[r]);
    }
    TR_FENCE();
    // Del^6 + Arakawa Jacobian (qgosubs.F:349-399); S / C / N rows gj-1 / gj / gj+1, w / e columns i-1 / i+1
#pragma unroll
    for (int t = 0; t < B; ++t) {
      const double d4A = d4[t], d4B = d4[t + 1], d4C = d4[t + 2];
      const double d4w = TR_WEST(d4B), d4e = TR_EAST(d4B);
      const double pS = pr[t], pC = pr[t + 1], pN = pr[t + 2];
      const double qS = qr[t], qC = qr[t + 1], qN = qr[t + 2];
      const double pSw = TR_WEST(pS), pSe = TR_EAST(pS), pCw = TR_WEST(pC), pCe = TR_EAST(pC), pNw = TR_WEST(pN), pNe = TR_EAST(pN);
      const double qSw = TR_WEST(qS), qSe = TR_EAST(qS), qCw = TR_WEST(qC), qCe = TR_EAST(qC), qNw = TR_WEST(qN), qNe = TR_EAST(qN);
      const double d6p = dxom2 * qg_five_point(d4A, d4w, d4e, d4C, d4B);
      const double diffus = PE.ah2fac[k] * d4B - PE.ah4fac[k] * d6p;
      double jac = qg_jac_head(qS, qCw, qCe, qN, pS, pCw, pCe, pN, pSw, pSe, pNw, pNe);
      jac = qg_jac_tail(jac, pS, pCw, pCe, pN, qSw, qSe, qNw, qNe);
      const double val = PE.adfaco * jac + diffus;
      dq[k][t] = cint ? val : 0.0; // dqdt = 0 on the wall columns (qgosubs.F:371,397)
      if (k == NL - 1) d2bot[t] = d2[t + 2];
      TR_PIN(dq[k][t]);
      TR_FENCE();
    }
    if (k + 1 < NL) {
      const double *pok = po0 + fs * (k + 1), *qok = qo0 + fs * (k + 1);
#pragma unroll
      for (int r = 0; r < B + 2; ++r) {
        pr[r] = tr_ld(pok, rowoff(jb - 1 + r) + lcol);
        qr[r] = tr_ld(qok, rowoff(jb - 1 + r) + lcol);
      }
      TR_FENCE();
    }
  }
  // ---- forcing, bottom drag, leapfrog, projection: tend_point's expressions (k_tend.h), every lane goes through ----
  // No vector-memory wait from the first store of the epilogue to the end of the strip: vmcnt counts loads AND stores and
  // retires them in order, the compiler does not count the write-through stores (inline asm), so any wait it places
  // behind one of them for a load of its own also waits for that store's acknowledgement.  The operands were requested
  // a layer's arithmetic ago; pinned here, their waits all stand in front of the first store
  // (tests/test_band_rows_epilogue_asm.py).
  // the epilogue's scalars, read once per strip: left inside the row loop each predicated block re-read its own
  // (s_load + s_waitcnt lgkmcnt(0), some twenty scalar round trips per strip)
  const double s_foh0 = PE.fohfac[0], s_foh1 = PE.fohfac[1], s_bdr = PE.bdrfac, s_beta = PE.beta, s_tdto = PE.tdto, s_fnot = PE.fnot;
  double s_ctl[NL * NL];
#pragma unroll
  for (int q = 0; q < NL * NL; ++q) s_ctl[q] = PE.ctl2m[q];
#pragma unroll
  for (int t = 0; t < B; ++t) {
    TR_PIN(e_wek[t]);
    if (ENT) TR_PIN(e_ent[ENT ? t : 0]);
    if (DDY) TR_PIN(e_ddy[DDY ? t : 0]);
#pragma unroll
    for (int kk = 0; kk < NL; ++kk) TR_PIN(e_qm[kk][t]);
  }
#pragma unroll
  for (int t = 0; t < B; ++t) {
    const int gj = jb + t;
    if (WALLS && gj > jr1) break; // (wave-uniform: the partial last band, never out of reach of the N wall row)
    const long o = (long)(gj - 1) * ldx + (gc - 1);
    // (a field the host knows to be all zero enters as a literal 0.0: the same expressions, the same bits)
    const double wek = e_wek[t], ent = ENT ? e_ent[ENT ? t : 0] : 0.0, ddy = DDY ? e_ddy[DDY ? t : 0] : 0.0;
    double qdot[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) qdot[k] = dq[k][t];
    qdot[0] = dq[0][t] + s_foh0 * (wek - ent);
    qdot[1] = dq[1][t] + s_foh1 * ent;
    qdot[NL - 1] = qdot[NL - 1] - s_bdr * d2bot[t];
    double ql[NL];
    const double betay = s_beta * e_yp[t]; // (yporel[gj - 1])
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const double qn = e_qm[k][t] + s_tdto * qdot[k]; // qom + tdto*qdot
      qg_pair_store_wt(PE.qnew + fs * k + o, qn, WALLS ? (own && gi <= nx - 1) : own);
      if (WALLS && own && gi == nx) PE.qnew[fs * k + o] = qn; // (the E wall column has no partner: the odd one out of 961)
      ql[k] = qn - betay;
    }
    ql[NL - 1] = ql[NL - 1] - ddy;
    double *dst = lds + ((t >> 1) * NL) * REG + (t & 1) * N + (gi - 2);
#pragma unroll
    for (int m = 0; m < NL; ++m) {
      double qmm = 0.0;
#pragma unroll
      for (int k = 0; k < NL; ++k) qmm = qmm + s_ctl[k + NL * m] * ql[k];
      if (own && cint) dst[m * REG] = s_fnot * qmm;
    }
  }
  // (a comment in the device assembly, no instruction: where this body ends - the compiler lays the two bodies out one
  //  behind the other with a flag in place of the else branch; tests/test_band_rows_epilogue_asm.py reads up to here)
  asm volatile("; tr_strip_end " TR_STR(TR_WALLS));
}
