// k_thomas_solve.inc - the body of the tridiagonal solve (see k_thomas.h), included into k_thomas (the handle's rows) and
// k_thomas_seg (one segment of a tall column).  Textual inclusion, not a device function: a by-value kernel argument
// that travels through a function parameter loses its address space (the loads through P.cycq became flat loads and
// k_thomas<16, 0, true> rose from 120 to 124 VGPRs), and the existing kernels are to compile to what they compiled to.
// The including kernel provides: template parameters R, PHASE, CYCA, KW; wrk, binf, rcb, wstride, ldw, jr0, jr1, nk,
// layer0, nblk (QG_TH_ARGS, or a segment's values); the kernel argument P; poff, send, slabDE (P's, or a segment's).
  QG_STAMP(1, 10);
  static_assert(TH_KW % KW == 0, "a workgroup's wavenumbers lie inside one block of the pivot tables");
  static_assert(KW % 2 == 0, "the write-through stores pair the lanes of neighbouring wavenumbers");
  // pitch TH_KW + 1: the scans read / write these arrays transposed ([lane][wv]: 64 lanes at a stride of one row);
  // at a pitch of 16 doubles = 128 B every lane hit the same pair of banks (SQ_LDS_BANK_CONFLICT was 55 % of the
  // kernel's LDS cycles)
  __shared__ double sC[TH_NC][KW + 1];
  __shared__ double sD[TH_NC][KW + 1];
  __shared__ double sIn[TH_NC][KW + 1];
  const int tid = threadIdx.x;
  if (CYCA && blockIdx.x == gridDim.x - 1) {
    // the extra workgroup: part A of the cyclic / atmospheric constraint algebra, one wave
    if (P.cycq && blockIdx.y == 0 && tid < 64) { // (cycq == nullptr: a stand-alone solve, part A runs in k_constr_cyc)
      double a4[QG_MAXL], b4[QG_MAXL];
      switch (P.g.nl) {
        case 2: constr_cyc_partA<2>(*P.cycq, tid, a4, b4); break;
        case 3: constr_cyc_partA<3>(*P.cycq, tid, a4, b4); break;
        default: constr_cyc_partA<4>(*P.cycq, tid, a4, b4); break;
      }
    }
    return;
  }
  QG_STAMP(1, 0);
  // KW = 8 (half a 128-byte line per row): the two workgroups that share the lines of a 16-wavenumber block go to the
  // SAME XCD - physical blocks b and b + 8 of every group of 16 (blocks are dealt round-robin over the 8 XCDs: the
  // grid's x extent is a multiple of 8 then) - so that one L2 fetches each line once.
  int bxl = (int)blockIdx.x;
  if (KW == 8) {
    const int nfull = (nk + KW - 1) / KW / 16 * 16; // (the grid's x extent less CYCA's extra workgroup, from a preloaded argument)
    if (bxl < nfull) bxl = (bxl & ~15) + 2 * (bxl & 7) + ((bxl >> 3) & 1);
  }
  const int kk = tid % KW;
  const int c = tid / KW;
  const int lane = tid & 63, wv = tid >> 6;
  const int k = bxl * KW + kk;
  const int kq = bxl * KW + wv; // wavenumber whose chunk maps this wave scans
  // (leading scalar arguments, preloaded into SGPRs: QG_TH_ARGS in qgcm_dev.h - the row loads below and the loads of
  //  rcb / binf are issued without waiting for the kernarg segment; aoc, ftnorm, poff and ptab are used after them)
  const int m = blockIdx.y + layer0;
  const int nr = jr1 - jr0 + 1; // local rows jr0..jr1  <->  r = 0..nr-1
  const bool kok = k < nk;
  const int r0 = c * R;
  const long mk = TH_MSG * ((long)m * ldw + kq);
  const double a = P.aoc, ft = P.ftnorm;

  // 32-bit element offsets from a uniform base (one scalar pointer + one VGPR per address)
  double *wbase = wrk + wstride * m + (long)(jr0 - 1) * ldw + bxl * KW;
  const unsigned off0 = (unsigned)(r0 * ldw + kk);
  // rows past the end of the slab: PHASE 0 (whole column, zero inflow at both ends) pads them with w = 0, b = 0 - the
  // forward values and the backward values of such rows are exactly 0, nothing of them is stored, and the sweeps need
  // no per-row predicate.  The slab phases publish the value LEAVING the slab, so there padded rows must be the
  // identity map: they keep the predicate.
  constexpr bool PRED = (PHASE != 0);
  double w[R], b[R];
  QG_STAMP(1, 11);
#pragma unroll
  for (int t = 0; t < R; ++t) {
    int r = r0 + t;
    const bool ok = kok && r < nr && PHASE != 4 && PHASE != 5;
    w[t] = ok ? wbase[off0 + (unsigned)(t * ldw)] : 0.0; // (unconditional loads at clamped offsets: 128 VGPRs + spills)
  }
  // pivots of this chunk (src/ocisubs.F:472-477, tabulated by the host): rows below rcb from the block's table,
  // the stationary value after that
  {
    const int tb = m * nblk + (bxl * KW) / TH_KW; // the tables are per block of TH_KW wavenumbers
    const int rcb_b = rcb[tb];
    const double binf_k = kok ? binf[(long)m * ldw + k] : 0.0;
#pragma unroll
    for (int t = 0; t < R; ++t) b[t] = binf_k;
    if (r0 < rcb_b) {
      const double *tab = P.ptab + (long)poff[tb] * TH_KW + (bxl * KW) % TH_KW + kk;
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const int r = r0 + t;
        const int rc = r < rcb_b ? r : rcb_b - 1;
        const double v = tab[rc * TH_KW];
        b[t] = (r < rcb_b && kok) ? v : binf_k;
      }
    }
    if (r0 + R > nr) {
#pragma unroll
      for (int t = 0; t < R; ++t)
        if (r0 + t >= nr) b[t] = 0.0;
    }
  }
  // values entering the slab: none (the inflows of the other ranks are added by k_thomas_corr), or the unit inflows
  // of the set-up phases
  const double uin = (PHASE == 4) ? 1.0 : 0.0, vin = (PHASE == 5) ? 1.0 : 0.0;
  // ---- forward: local affine maps (zero inflow); rows past the slab are the identity (PRED) or the zero map (PHASE 0)
  double C = 0.0, D = 1.0;
#pragma unroll
  for (int t = 0; t < R; ++t) {
    w[t] *= b[t];
    b[t] *= a;
  }
#pragma unroll
  for (int t = 0; t < R; ++t) {
    if (!PRED || r0 + t < nr) {
      C = __builtin_fma(-b[t], C, w[t]);
      D = -b[t] * D;
    }
  }
  QG_STAMP(1, 1);
  sC[c][kk] = C;
  sD[c][kk] = D;
  __syncthreads();
  QG_STAMP(1, 2);
  double Cs = sC[lane][wv], Ds = sD[lane][wv];
  affine_scan(Cs, Ds, lane);
  // lane 63 holds the composition of all chunks: zero-inflow end value and slab gain
  const double Cf_tot = __shfl(Cs, 63), D_tot = __shfl(Ds, 63);
  {
    // value entering chunk `lane` = scanned map of chunk lane-1 applied to uin
    double Cprev = th_dpp<0x138>(Cs), Dprev = th_dpp<0x138>(Ds); // wave_shr:1 (lane 0 is not used)
    sIn[lane][wv] = (lane == 0) ? uin : Cprev + Dprev * uin;
  }
  __syncthreads();
  QG_STAMP(1, 3);
  double u = sIn[c][kk];
#pragma unroll
  for (int t = 0; t < R; ++t) {
    if (!PRED || r0 + t < nr) {
      u = __builtin_fma(-b[t], u, w[t]);
      w[t] = u;
    }
  }
  // ---- backward: v_r = u_r - a*bet_r*v_{r+1} ------------------------------
  // (the chunk gain is formed again, in descending order)
  C = 0.0;
  D = 1.0;
#pragma unroll
  for (int t = R - 1; t >= 0; --t) {
    if (!PRED || r0 + t < nr) {
      C = __builtin_fma(-b[t], C, w[t]);
      D = -b[t] * D;
    }
  }
  sC[c][kk] = C; // safe without a barrier: every wave read the forward maps in sC / sD before the barrier above
  sD[c][kk] = D;
  __syncthreads();
  QG_STAMP(1, 4);
  // sweep order is last chunk first: lane l stands for chunk 63-l
  const int cr = 63 - lane;
  Cs = sC[cr][wv];
  Ds = sD[cr][wv];
  affine_scan(Cs, Ds, lane);
  const double Cb_tot = __shfl(Cs, 63); // first value of the zero-inflow backward sweep
  {
    double Cprev = th_dpp<0x138>(Cs), Dprev = th_dpp<0x138>(Ds); // wave_shr:1 (lane 0 is not used)
    sIn[cr][wv] = (lane == 0) ? vin : Cprev + Dprev * vin;
  }
  __syncthreads();
  QG_STAMP(1, 5);
  double v = sIn[c][kk];
  double colsum = 0.0;
#pragma unroll
  for (int t = R - 1; t >= 0; --t) {
    if (!PRED || r0 + t < nr) {
      v = __builtin_fma(-b[t], v, w[t]);
      w[t] = v;
      colsum += v;
    }
  }
  QG_STAMP(1, 6);
  {
    if (R % 2 == 0) {
      // 16-byte write-through stores (qgcm_dev.h: all of this kernel's stores come at its very end): the lanes of two
      // neighbouring wavenumbers swap one value per pair of rows, the even lane then stores row t for both, the odd
      // lane row t + 1 (columns k - 1, k).  A column past nk is a padding column of the row (ldw = nk rounded up).
      const bool odd = (kk & 1) != 0;
      const bool pok = odd ? (k - 1 < nk) : kok; // the pair's first column exists
      double *cbase = wbase + (odd ? off0 - 1 : off0);
#pragma unroll
      for (int t = 0; t < R; t += 2) {
        const double mine0 = ft * w[t], mine1 = ft * w[t + 1];
        const double give = odd ? mine0 : mine1;
        int lo = __double2loint(give), hi = __double2hiint(give);
        lo = __builtin_amdgcn_update_dpp(0, lo, 0xb1, 0xf, 0xf, true); // quad_perm [1,0,3,2]
        hi = __builtin_amdgcn_update_dpp(0, hi, 0xb1, 0xf, 0xf, true);
        const double got = __hiloint2double(hi, lo);
        const int r = r0 + t + (odd ? 1 : 0);
        if (pok && r < nr) qg_store16_wt(cbase + (unsigned)((t + (odd ? 1 : 0)) * ldw), odd ? got : mine0, odd ? mine1 : got);
      }
    } else {
#pragma unroll
      for (int t = 0; t < R; ++t) {
        int r = r0 + t;
        if (kok && r < nr) wbase[off0 + (unsigned)(t * ldw)] = ft * w[t];
      }
    }
  }
  QG_STAMP(1, 7);
  QG_STAMP_DRAIN();
  QG_STAMP(1, 8);
  if (CYCA && PHASE == 0 && P.ybnd && k == 0) { // (cyclic instantiation only: the box kernel has no register to spare)
    // cyclic constraints: the zonal-mean solution next to the two zonal boundaries (rows 2 and nypo-1) goes to a side
    // buffer, so that part B of the constraint algebra does not have to read wrk - which the in-place inverse rows of
    // the generic sizes overwrite - and can ride in that launch
#pragma unroll
    for (int t = 0; t < R; ++t) {
      if (r0 + t == 0) P.ybnd[2 * m] = ft * w[t];
      if (r0 + t == nr - 1) P.ybnd[2 * m + 1] = ft * w[t];
    }
  }
  // column sum of this slab: chunks in a fixed order (lanes of wave wv = chunks of wavenumber kq)
  sC[c][kk] = colsum;
  __syncthreads();
  double tot = sC[lane][wv];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
  if (lane != 0 || kq >= nk) return;
  double *cst = slabDE + 4 * ((long)m * ldw + kq); // D, E, SP, SQ of this slab
  if (PHASE == 0) {
    P.ksum[(long)m * ldw + kq] = ft * tot;
  } else if (PHASE == 1) {
    send[mk] = Cf_tot;
    send[mk + 1] = Cb_tot;
    send[mk + 2] = tot;
  } else if (PHASE == 4) {
    cst[0] = D_tot;
    cst[1] = Cb_tot;
    cst[2] = tot;
  } else {
    cst[3] = tot;
  }
