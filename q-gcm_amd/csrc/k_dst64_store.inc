// k_dst64_store.inc - epilogue of a forward row pair (k_dst64, k_tend_rows): the two transformed rows go from the wave's
// LDS buffer to wrk in 16-byte write-through stores.  Textual inclusion: as a function template k_tend_rows compiled to
// another schedule (DESIGN 9).  The including kernel provides: the row length N (constexpr); lane; raw (the transform
// buffer as dst64_back leaves it, const double *); rowa, rowb (the rows of wrk); has_b (the pair has its second row).
  constexpr int NP = N + N / 16;
  {
    constexpr int NU = (N / 2 + 63) / 64;
    // all LDS reads of the two output rows first, then the global stores (one exposed LDS round trip instead of 2 NU)
    double2 oa[NU], ob[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int t = lane + 64 * u;
      const int tc = t < N / 2 ? t : N / 2 - 1;
      const int i = 2 * tc + ((2 * tc) >> 4); // 2t and 2t+1 share a 16-group: consecutive after padding
      oa[u] = double2{raw[i], raw[i + 1]};
      ob[u] = double2{raw[NP + i], raw[NP + i + 1]};
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int t = lane + 64 * u;
      if (t < N / 2) { // (write-through: qgcm_dev.h)
        qg_store16_wt(rowa + 2 * t, oa[u].x, oa[u].y);
        if (has_b) qg_store16_wt(rowb + 2 * t, ob[u].x, ob[u].y);
      }
    }
  }
