!-----------------------------------------------------------------------
! qgcm_hip_iface - ISO_C_BINDING view of include/qgcm_hip.h
!
! One interface per C entry point; the derived type mirrors
! struct qgcm_hip_params field for field (QGCM_HIP_MAXL = 8).
!-----------------------------------------------------------------------
module qgcm_hip_iface
  use iso_c_binding
  implicit none
  public

  integer, parameter :: QGCM_HIP_MAXL = 8

  type, bind(C) :: qgcm_hip_params
    integer(c_int) :: nxpo, nypo, nlo, cyclic
    real(c_double) :: fnot, beta, dxo, dyo, tdto, delek, bccooc
    real(c_double) :: ah2oc(QGCM_HIP_MAXL), ah4oc(QGCM_HIP_MAXL)
    real(c_double) :: hoc(QGCM_HIP_MAXL), gpoc(QGCM_HIP_MAXL)
    real(c_double) :: amatoc(QGCM_HIP_MAXL*QGCM_HIP_MAXL)
    real(c_double) :: ctl2moc(QGCM_HIP_MAXL*QGCM_HIP_MAXL)
    real(c_double) :: ctm2loc(QGCM_HIP_MAXL*QGCM_HIP_MAXL)
    real(c_double) :: rdm2oc(QGCM_HIP_MAXL)
    real(c_double) :: aoc
    integer(c_int) :: slab_g0, slab_g1
    integer(c_int) :: atmos   ! 1: the handle is the atmospheric channel (qgastep / atinvq / atqzbd)
  end type qgcm_hip_params

  ! struct qgcm_hip_oml_params: run-time parameters of the ocean mixed layer
  type, bind(C) :: qgcm_hip_oml_params
    real(c_double) :: hmoc, toc1, toc2, st2d, st4d, ycexp, rrcpoc, tsbdy, tnbdy
    integer(c_int) :: sb_flag, nb_flag   ! sb_hflux, nb_hflux of the C struct (those names are cpp macros in reference builds)
  end type qgcm_hip_oml_params

  ! struct qgcm_hip_tav_params: constants of tavocn
  type, bind(C) :: qgcm_hip_tav_params
    real(c_double) :: hmoc, ycexp, tsbdy, tnbdy
    integer(c_int) :: sb_flag, nb_flag   ! sb_hflux, nb_hflux of the C struct
  end type qgcm_hip_tav_params

  ! struct qgcm_hip_atm_mon_params: constants of the atmosphere monitors (qgcm_hip_set_atm_mon_params)
  type, bind(C) :: qgcm_hip_atm_mon_params
    real(c_double) :: rhoat, cpat, hmat, davgat
    real(c_double) :: aup(QGCM_HIP_MAXL-1)   ! Aup(nla, 1..nla-1)
    real(c_double) :: bup, cup, dup          ! Bup(nla), Cup(nla), Dup(nla)
    integer(c_int) :: nx1, ny1, nxaooc, nyaooc
  end type qgcm_hip_atm_mon_params

  ! struct qgcm_hip_xforc_params: constants and bicubic weight tables of the momentum half of xforc
  ! (qgcm_hip_xforc_init); stb** = c_loc of MODULE xfosubs' tables (16, 0:ndxr, 0:ndxr)
  type, bind(C) :: qgcm_hip_xforc_params
    integer(c_int) :: ndxr, nx1, ny1, nxaooc, nyaooc
    real(c_double) :: cdat, raoro, hmat, hmoc, bccoat, bccooc
    integer(c_int) :: udiff_flag   ! tau_udiff of the C struct (that name is a cpp macro in reference builds)
    type(c_ptr) :: stbbb, stbus, stbvs, stbun, stbvn
  end type qgcm_hip_xforc_params

  ! struct qgcm_hip_aml_params: constants of the atmospheric mixed layer (qgcm_hip_aml_init); xc1ast, dtopat = c_loc
  ! of MODULE atconst's arrays, or c_null_ptr for zeros
  type, bind(C) :: qgcm_hip_aml_params
    real(c_double) :: hmat, hmamin, hmadmp, rrcpat, tat1, tat2, xcexp, at2d, at4d, ahmd
    real(c_double) :: aface(QGCM_HIP_MAXL-1)
    real(c_double) :: bface, cface, dface
    type(c_ptr) :: xc1ast, dtopat
  end type qgcm_hip_aml_params

  ! struct qgcm_hip_xforc_heat_params: constants of the heat half of xforc (qgcm_hip_xforc_heat_init); fsa, fso = c_loc
  ! of the tables fsprim(ytarel), fsprim(ytorel); xta, yta, xto, yto = c_loc of MODULE atconst's / occonst's vectors
  type, bind(C) :: qgcm_hip_xforc_heat_params
    real(c_double) :: xlamda, D0up, Dmup, Dmdown, Adown11, Bmup, B1down, Cmup, C1down, hmadmp, hmat
    type(c_ptr) :: fsa, fso, xta, yta, xto, yto
  end type qgcm_hip_xforc_heat_params

  ! struct qgcm_hip_xforc_sst_params: the heat half of xforc without an ocean (atmos_only; qgcm_hip_xforc_sst_init):
  ! the constants and fsa, xta, yta, xto, yto as above; dxo, dyo = the spacing of the SST grid; sst = c_loc of the
  ! (nxto, nyto) field that is read once and held
  type, bind(C) :: qgcm_hip_xforc_sst_params
    real(c_double) :: xlamda, D0up, Dmup, Dmdown, Adown11, Bmup, B1down, Cmup, C1down, hmadmp, hmat
    type(c_ptr) :: fsa, xta, yta, xto, yto
    real(c_double) :: dxo, dyo
    type(c_ptr) :: sst
  end type qgcm_hip_xforc_sst_params

  interface
    integer(c_int) function qgcm_hip_create(h, prm, device) bind(C, name='qgcm_hip_create')
      import :: c_ptr, c_int, qgcm_hip_params
      type(c_ptr), intent(out) :: h
      type(qgcm_hip_params), intent(in) :: prm
      integer(c_int), value :: device
    end function
    integer(c_int) function qgcm_hip_destroy(h) bind(C, name='qgcm_hip_destroy')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    type(c_ptr) function qgcm_hip_last_error() bind(C, name='qgcm_hip_last_error')
      import :: c_ptr
    end function
    integer(c_int) function qgcm_hip_set_grid(h, yporel, bd2oc, ddynoc) bind(C, name='qgcm_hip_set_grid')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: yporel(*), bd2oc(*), ddynoc(*)
    end function
    integer(c_int) function qgcm_hip_set_geometry(h, yporel, ddynoc) bind(C, name='qgcm_hip_set_geometry')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: yporel(*), ddynoc(*)
    end function
    integer(c_int) function qgcm_hip_set_homog_box(h, ochom, cdiffo, cdhoc) bind(C, name='qgcm_hip_set_homog_box')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: ochom(*), cdiffo(*), cdhoc(*)
    end function
    integer(c_int) function qgcm_hip_set_homog_cyc(h, pch1oc, pch2oc, pbhoc, aipcho, hc1soc, hc2soc, hc1noc, hc2noc, &
                                                   hbsioc, aipbho) bind(C, name='qgcm_hip_set_homog_cyc')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: pch1oc(*), pch2oc(*), pbhoc(*), aipcho(*), hc1soc(*), hc2soc(*), hc1noc(*), hc2noc(*)
      real(c_double), value :: hbsioc, aipbho
    end function
    integer(c_int) function qgcm_hip_abi_version() bind(C, name='qgcm_hip_abi_version')
      import :: c_int
    end function
    integer(c_int) function qgcm_hip_set_sponge(h, r_spl, c1_spl) bind(C, name='qgcm_hip_set_sponge')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: r_spl(*)
      real(c_double), value :: c1_spl
    end function
    integer(c_int) function qgcm_hip_set_cyc_forcing(h, txisoc, txinoc, enisoc, eninoc) bind(C, name='qgcm_hip_set_cyc_forcing')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), value :: txisoc, txinoc
      real(c_double), intent(in) :: enisoc(*), eninoc(*)
    end function
    integer(c_int) function qgcm_hip_set_state(h, po, pom, qo, qom) bind(C, name='qgcm_hip_set_state')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: po(*), pom(*), qo(*), qom(*)
    end function
    integer(c_int) function qgcm_hip_get_state(h, po, pom, qo, qom) bind(C, name='qgcm_hip_get_state')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: po(*), pom(*), qo(*), qom(*)
    end function
    integer(c_int) function qgcm_hip_set_forcing(h, wekpo, entoc, xon) bind(C, name='qgcm_hip_set_forcing')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: wekpo(*), entoc(*), xon(*)
    end function
    integer(c_int) function qgcm_hip_set_scalars(h, scal) bind(C, name='qgcm_hip_set_scalars')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: scal(*)
    end function
    integer(c_int) function qgcm_hip_get_scalars(h, scal) bind(C, name='qgcm_hip_get_scalars')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: scal(*)
    end function
    integer(c_int) function qgcm_hip_get_monitors(h, ermas, emfr) bind(C, name='qgcm_hip_get_monitors')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: ermas(*), emfr(*)
    end function
    integer(c_int) function qgcm_hip_qgostep(h) bind(C, name='qgcm_hip_qgostep')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_ocinvq(h) bind(C, name='qgcm_hip_ocinvq')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_ocqbdy(h) bind(C, name='qgcm_hip_ocqbdy')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    ! "call ocqbdy (q, p)" / "call atqzbd (q, p)" on host arrays (start-up calls, src/q-gcm.F:724-725, 743-744)
    integer(c_int) function qgcm_hip_ocqbdy_host(h, q, p) bind(C, name='qgcm_hip_ocqbdy_host')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(inout) :: q(*)
      real(c_double), intent(in) :: p(*)
    end function
    ! atmosphere path (handles created with prm%atmos = 1): src/q-gcm.F:1262-1268
    integer(c_int) function qgcm_hip_qgastep(h) bind(C, name='qgcm_hip_qgastep')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_atinvq(h) bind(C, name='qgcm_hip_atinvq')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_atqzbd(h) bind(C, name='qgcm_hip_atqzbd')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_get_bsums(h, b) bind(C, name='qgcm_hip_get_bsums')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: b(*)
    end function
    integer(c_int) function qgcm_hip_coupled_steps(oc, atm, nt0, n, nstr) bind(C, name='qgcm_hip_coupled_steps')
      import :: c_ptr, c_int
      type(c_ptr), value :: oc, atm
      integer(c_int), value :: nt0, n, nstr
    end function
    ! a handle's share of the GPU's compute units when two handles step side by side (qgcm_hip_coupled_steps)
    integer(c_int) function qgcm_hip_set_cu_range(h, first, count) bind(C, name='qgcm_hip_set_cu_range')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: first, count
    end function
    ! start-up / restart arithmetic and the progress sample on the device (src/q-gcm.F:711-731, 1933-2066;
    ! src/xfosubs.F:566-645)
    integer(c_int) function qgcm_hip_init_from_p(h) bind(C, name='qgcm_hip_init_from_p')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_wekpo_from_tau(h, tauxo, tauyo) bind(C, name='qgcm_hip_wekpo_from_tau')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: tauxo(*), tauyo(*)
    end function
    integer(c_int) function qgcm_hip_prsamp(h, out) bind(C, name='qgcm_hip_prsamp')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: out(*)
    end function
    integer(c_int) function qgcm_hip_lf_average(h) bind(C, name='qgcm_hip_lf_average')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_steps(h, s0, n) bind(C, name='qgcm_hip_steps')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: s0, n
    end function
    integer(c_int) function qgcm_hip_sync(h) bind(C, name='qgcm_hip_sync')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_helmholtz(h, wrk, boc) bind(C, name='qgcm_hip_helmholtz')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(inout) :: wrk(*)
      real(c_double), intent(in) :: boc(*)
    end function
    ! ocean mixed layer: "call oml" (src/q-gcm.F:1232) on the device
    integer(c_int) function qgcm_hip_oml_init(h, prm) bind(C, name='qgcm_hip_oml_init')
      import :: c_ptr, c_int, qgcm_hip_oml_params
      type(c_ptr), value :: h
      type(qgcm_hip_oml_params), intent(in) :: prm
    end function
    integer(c_int) function qgcm_hip_oml_set_state(h, sst, sstm) bind(C, name='qgcm_hip_oml_set_state')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: sst(*), sstm(*)
    end function
    integer(c_int) function qgcm_hip_oml_get_state(h, sst, sstm) bind(C, name='qgcm_hip_oml_get_state')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: sst(*), sstm(*)
    end function
    integer(c_int) function qgcm_hip_oml_set_forcing(h, fnetoc, wekto, tauxo, tauyo) bind(C, name='qgcm_hip_oml_set_forcing')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: fnetoc(*), wekto(*), tauxo(*), tauyo(*)
    end function
    integer(c_int) function qgcm_hip_oml(h) bind(C, name='qgcm_hip_oml')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_oml_get_diag(h, entoc, diag) bind(C, name='qgcm_hip_oml_get_diag')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: entoc(*), diag(5)
    end function
    ! validity scan: ocean part of "call valids (solnok)" (src/q-gcm.F:1278) on the device
    integer(c_int) function qgcm_hip_set_dtopoc(h, dtopoc) bind(C, name='qgcm_hip_set_dtopoc')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: dtopoc(*)
    end function
    integer(c_int) function qgcm_hip_valids(h, out, solnok) bind(C, name='qgcm_hip_valids')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: out(*)
      integer(c_int), intent(out) :: solnok
    end function
    ! y-slab runs, one process per GPU: rendezvous id (rank 0), communicator, whole distributed steps
    ! (the library issues the RCCL exchanges itself; include/qgcm_hip.h)
    integer(c_int) function qgcm_hip_comm_unique_id(id, nbytes) bind(C, name='qgcm_hip_comm_unique_id')
      import :: c_int, c_char
      character(kind=c_char), intent(out) :: id(*)
      integer(c_int), value :: nbytes
    end function
    integer(c_int) function qgcm_hip_comm_init(h, id, nbytes, rank, nranks) bind(C, name='qgcm_hip_comm_init')
      import :: c_ptr, c_int, c_char
      type(c_ptr), value :: h
      character(kind=c_char), intent(in) :: id(*)
      integer(c_int), value :: nbytes, rank, nranks
    end function
    integer(c_int) function qgcm_hip_slab_steps(h, s0, n) bind(C, name='qgcm_hip_slab_steps')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: s0, n
    end function
    ! the coupled window on a y-slab ocean with the library as the driver (DESIGN 6t): after qgcm_hip_comm_init and the
    ! xforc set-ups of the slab and its replica of the atmosphere; collective, asynchronous
    integer(c_int) function qgcm_hip_slab_coupled_init(oc, atm) bind(C, name='qgcm_hip_slab_coupled_init')
      import :: c_ptr, c_int
      type(c_ptr), value :: oc, atm
    end function
    integer(c_int) function qgcm_hip_slab_coupled_steps(oc, atm, nt0, n, nstr, xforc) &
        bind(C, name='qgcm_hip_slab_coupled_steps')
      import :: c_ptr, c_int
      type(c_ptr), value :: oc, atm
      integer(c_int), value :: nt0, n, nstr, xforc
    end function
    ! own exchanges: the right-hand-side independent part of the slab summaries, once after set_grid
    integer(c_int) function qgcm_hip_thomas_const_len(h) bind(C, name='qgcm_hip_thomas_const_len')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_thomas_consts(h, dst_dev) bind(C, name='qgcm_hip_thomas_consts')
      import :: c_ptr, c_int
      type(c_ptr), value :: h, dst_dev
    end function
    integer(c_int) function qgcm_hip_set_thomas_consts(h, gath_dev, nranks) bind(C, name='qgcm_hip_set_thomas_consts')
      import :: c_ptr, c_int
      type(c_ptr), value :: h, gath_dev
      integer(c_int), value :: nranks
    end function
    ! the row plan of a zonally cyclic ocean: nxto = P * L (host code; forced_P = 0: the default rule), and a handle's
    integer(c_int) function qgcm_hip_row_split(nxto, forced_P, P, L) bind(C, name='qgcm_hip_row_split')
      import :: c_int
      integer(c_int), value :: nxto, forced_P
      integer(c_int) :: P, L
    end function
    integer(c_int) function qgcm_hip_row_plan(h, P, L) bind(C, name='qgcm_hip_row_plan')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int) :: P, L
    end function
    integer(c_int) function qgcm_hip_comm_probe(h, reps, us) bind(C, name='qgcm_hip_comm_probe')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      integer(c_int), value :: reps
      real(c_double), intent(out) :: us(3)
    end function
    integer(c_int) function qgcm_hip_comm_set_halo_p2p(h, on) bind(C, name='qgcm_hip_comm_set_halo_p2p')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: on
    end function
    integer(c_int) function qgcm_hip_comm_set_overlap(h, on) bind(C, name='qgcm_hip_comm_set_overlap')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: on
    end function
    ! time averages of the ocean (include/qgcm_hip.h): running mean of po (avg_ocn_k247 / ocnc_avgout_k247) and
    ! tavocn / tavout; fields(16) holds c_loc of the outputs wanted (c_null_ptr = skip), in the header's order
    integer(c_int) function qgcm_hip_poavg_enable(h, on) bind(C, name='qgcm_hip_poavg_enable')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: on
    end function
    integer(c_int) function qgcm_hip_poavg_out(h, po_avg, nsum, reset) bind(C, name='qgcm_hip_poavg_out')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: po_avg(*)
      integer(c_int), intent(out) :: nsum
      integer(c_int), value :: reset
    end function
    integer(c_int) function qgcm_hip_set_tav_params(h, p) bind(C, name='qgcm_hip_set_tav_params')
      import :: c_ptr, c_int, qgcm_hip_tav_params
      type(c_ptr), value :: h
      type(qgcm_hip_tav_params), intent(in) :: p
    end function
    integer(c_int) function qgcm_hip_set_tav_fields(h, fnetoc) bind(C, name='qgcm_hip_set_tav_fields')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: fnetoc(*)
    end function
    integer(c_int) function qgcm_hip_tavocn(h) bind(C, name='qgcm_hip_tavocn')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_tav_reset(h) bind(C, name='qgcm_hip_tav_reset')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_tav_out(h, fields, nsumoc) bind(C, name='qgcm_hip_tav_out')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      type(c_ptr), intent(in) :: fields(16)
      integer(c_int), intent(out) :: nsumoc
    end function
    ! periodic ocean dumps (qocdiag_out, ocnc_out; DESIGN 6g)
    integer(c_long) function qgcm_hip_qocdiag_len(h, nsko) bind(C, name='qgcm_hip_qocdiag_len')
      import :: c_ptr, c_int, c_long
      type(c_ptr), value :: h
      integer(c_int), value :: nsko
    end function
    integer(c_int) function qgcm_hip_qocdiag(h, nsko, out) bind(C, name='qgcm_hip_qocdiag')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      integer(c_int), value :: nsko
      real(c_double), intent(out) :: out(*)
    end function
    integer(c_int) function qgcm_hip_qocdiag_schedule(h, nsko, every, capacity) bind(C, name='qgcm_hip_qocdiag_schedule')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: nsko, every, capacity
    end function
    ! out, steps_out: c_loc of the caller's arrays, or c_null_ptr (steps_out not wanted; out with max <= 0, the query)
    integer(c_int) function qgcm_hip_qocdiag_read(h, out, steps_out, max, nread) bind(C, name='qgcm_hip_qocdiag_read')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      type(c_ptr), value :: out, steps_out
      integer(c_int), value :: max
      integer(c_int), intent(out) :: nread
    end function
    integer(c_long) function qgcm_hip_ocnc_sample_len(h, nsko, outfloc) bind(C, name='qgcm_hip_ocnc_sample_len')
      import :: c_ptr, c_int, c_long
      type(c_ptr), value :: h
      integer(c_int), value :: nsko
      integer(c_int), intent(in) :: outfloc(7)
    end function
    integer(c_int) function qgcm_hip_ocnc_sample(h, nsko, outfloc, out) bind(C, name='qgcm_hip_ocnc_sample')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      integer(c_int), value :: nsko
      integer(c_int), intent(in) :: outfloc(7)
      real(c_double), intent(out) :: out(*)
    end function
    integer(c_int) function qgcm_hip_subsample_rows(h, nsko, mp0, mp1, mt0, mt1) bind(C, name='qgcm_hip_subsample_rows')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: nsko
      integer(c_int), intent(out) :: mp0, mp1, mt0, mt1
    end function
    ! atmosphere monitors and valids (the atmosphere half of monnc_comp, courat, valids; DESIGN 6h)
    integer(c_int) function qgcm_hip_set_atm_mon_params(h, p) bind(C, name='qgcm_hip_set_atm_mon_params')
      import :: c_ptr, c_int, qgcm_hip_atm_mon_params
      type(c_ptr), value :: h
      type(qgcm_hip_atm_mon_params), intent(in) :: p
    end function
    ! c_loc of the caller's arrays, or c_null_ptr to leave a field unchanged
    integer(c_int) function qgcm_hip_set_atm_monitor_fields(h, wekta, tauxa, tauya, ast, hmixa, uekat, vekat) &
        bind(C, name='qgcm_hip_set_atm_monitor_fields')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      type(c_ptr), value :: wekta, tauxa, tauya, ast, hmixa, uekat, vekat
    end function
    integer(c_int) function qgcm_hip_atm_monitor_len(h) bind(C, name='qgcm_hip_atm_monitor_len')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_atm_monitors(h, out) bind(C, name='qgcm_hip_atm_monitors')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: out(*)
    end function
    integer(c_int) function qgcm_hip_atm_valids(h, out, solnok) bind(C, name='qgcm_hip_atm_valids')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: out(12)
      integer(c_int), intent(out) :: solnok
    end function
    ! area averages and the CFL check (areavg, cfltry; DESIGN 6m).  Not called by the drop-in, which still pulls the
    ! state before areavg / cfltry (INTEGRATION.md)
    integer(c_int) function qgcm_hip_areavg_init(h, n, i1, i2, j1, j2, facw, face, facs, facn) &
        bind(C, name='qgcm_hip_areavg_init')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      integer(c_int), value :: n
      integer(c_int), intent(in) :: i1(*), i2(*), j1(*), j2(*)
      real(c_double), intent(in) :: facw(*), face(*), facs(*), facn(*)
    end function
    integer(c_int) function qgcm_hip_areavg_count(h) bind(C, name='qgcm_hip_areavg_count')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    ! c_loc of num(n), den(n), or c_null_ptr
    integer(c_int) function qgcm_hip_areavg(h, avg, num, den) bind(C, name='qgcm_hip_areavg')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: avg(*)
      type(c_ptr), value :: num, den
    end function
    integer(c_int) function qgcm_hip_areavg_part_len(h) bind(C, name='qgcm_hip_areavg_part_len')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_areavg_part(h, send_dev) bind(C, name='qgcm_hip_areavg_part')
      import :: c_ptr, c_int
      type(c_ptr), value :: h, send_dev
    end function
    integer(c_int) function qgcm_hip_areavg_combine(h, gath_dev, nranks, avg, num, den) &
        bind(C, name='qgcm_hip_areavg_combine')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h, gath_dev
      integer(c_int), value :: nranks
      real(c_double), intent(out) :: avg(*)
      type(c_ptr), value :: num, den
    end function
    integer(c_int) function qgcm_hip_cfl_len(h) bind(C, name='qgcm_hip_cfl_len')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    ! maxima(2*(nl+1)), nbad(2*(nl+1)), loc(2, 2*(nl+1)) = (i, j) of every maximum
    integer(c_int) function qgcm_hip_cfl(h, cflcrit, maxima, nbad, loc) bind(C, name='qgcm_hip_cfl')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), value :: cflcrit
      real(c_double), intent(out) :: maxima(*)
      integer(c_int), intent(out) :: nbad(*), loc(2,*)
    end function
    integer(c_int) function qgcm_hip_cfl_part_len(h) bind(C, name='qgcm_hip_cfl_part_len')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_cfl_part(h, cflcrit, send_dev) bind(C, name='qgcm_hip_cfl_part')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h, send_dev
      real(c_double), value :: cflcrit
    end function
    integer(c_int) function qgcm_hip_cfl_combine(h, gath_dev, nranks, cflcrit, maxima, nbad, loc) &
        bind(C, name='qgcm_hip_cfl_combine')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h, gath_dev
      integer(c_int), value :: nranks
      real(c_double), value :: cflcrit
      real(c_double), intent(out) :: maxima(*)
      integer(c_int), intent(out) :: nbad(*), loc(2,*)
    end function
    ! time averages and periodic dump of the atmosphere (tavatm / tavout, atnc_out; DESIGN 6i).  Not called by the
    ! drop-in, which still pulls the state before tavatm / atnc_out (INTEGRATION.md)
    integer(c_int) function qgcm_hip_set_atm_tav_fields(h, fnetat) bind(C, name='qgcm_hip_set_atm_tav_fields')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: fnetat(*)
    end function
    integer(c_int) function qgcm_hip_tavatm(h) bind(C, name='qgcm_hip_tavatm')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_atm_tav_reset(h) bind(C, name='qgcm_hip_atm_tav_reset')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_atm_tav_out(h, fields, nsumat) bind(C, name='qgcm_hip_atm_tav_out')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      type(c_ptr), intent(in) :: fields(15)
      integer(c_int), intent(out) :: nsumat
    end function
    integer(c_int) function qgcm_hip_tavatm_schedule(h, every, phase) bind(C, name='qgcm_hip_tavatm_schedule')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: every, phase
    end function
    integer(c_long) function qgcm_hip_atnc_sample_len(h, nska, outflat) bind(C, name='qgcm_hip_atnc_sample_len')
      import :: c_ptr, c_int, c_long
      type(c_ptr), value :: h
      integer(c_int), value :: nska
      integer(c_int), intent(in) :: outflat(7)
    end function
    integer(c_int) function qgcm_hip_atnc_sample(h, nska, outflat, out) bind(C, name='qgcm_hip_atnc_sample')
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      integer(c_int), value :: nska
      integer(c_int), intent(in) :: outflat(7)
      real(c_double), intent(out) :: out(*)
    end function
    ! covariance matrices (DESIGN 6j): covini / covocn / covatm; packed index k = i(i+1)/2 + j (0-based)
    integer(c_int) function qgcm_hip_cov_init(h, nsi, rank, nranks) bind(C, name='qgcm_hip_cov_init')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: nsi, rank, nranks
    end function
    integer(c_int) function qgcm_hip_cov_size(h, nvar, nmat, k0, k1) bind(C, name='qgcm_hip_cov_size')
      import :: c_ptr, c_int, c_long
      type(c_ptr), value :: h
      integer(c_long), intent(out) :: nvar, nmat, k0, k1
    end function
    integer(c_int) function qgcm_hip_cov_add(h) bind(C, name='qgcm_hip_cov_add')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_cov_reset(h) bind(C, name='qgcm_hip_cov_reset')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_cov_out(h, which, avg, swt, nunit, k0, count, cov) bind(C, name='qgcm_hip_cov_out')
      import :: c_ptr, c_int, c_long, c_double
      type(c_ptr), value :: h
      integer(c_int), value :: which
      real(c_double), intent(out) :: avg(*), swt
      integer(c_long), intent(out) :: nunit
      integer(c_long), value :: k0, count
      real(c_double), intent(out) :: cov(*)
    end function
    integer(c_int) function qgcm_hip_cov_schedule(h, every, phase) bind(C, name='qgcm_hip_cov_schedule')
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: every, phase
    end function
    integer(c_long) function qgcm_hip_cov_part_len(h) bind(C, name='qgcm_hip_cov_part_len')
      import :: c_ptr, c_long
      type(c_ptr), value :: h
    end function
    integer(c_int) function qgcm_hip_cov_part(h, send_dev) bind(C, name='qgcm_hip_cov_part')
      import :: c_ptr, c_int
      type(c_ptr), value :: h, send_dev
    end function
    integer(c_int) function qgcm_hip_cov_combine(h, gath_dev, nranks) bind(C, name='qgcm_hip_cov_combine')
      import :: c_ptr, c_int
      type(c_ptr), value :: h, gath_dev
      integer(c_int), value :: nranks
    end function
    ! momentum half of xforc on the device (src/xfosubs.F:137-709); oc = c_null_ptr: the atmos_only half
    integer(c_int) function qgcm_hip_xforc_init(oc, atm, prm) bind(C, name='qgcm_hip_xforc_init')
      import :: c_ptr, c_int, qgcm_hip_xforc_params
      type(c_ptr), value :: oc, atm
      type(qgcm_hip_xforc_params), intent(in) :: prm
    end function
    integer(c_int) function qgcm_hip_xforc(oc, atm) bind(C, name='qgcm_hip_xforc')
      import :: c_ptr, c_int
      type(c_ptr), value :: oc, atm
    end function
    ! every field is a c_ptr (c_loc of the host array, or c_null_ptr to skip it); txi: txisat, txinat, txisoc, txinoc
    integer(c_int) function qgcm_hip_xforc_get(oc, atm, tauxa, tauya, uekat, vekat, wekta, wekpa, tauxo, tauyo, wekto, &
                                               wekpo, txi) bind(C, name='qgcm_hip_xforc_get')
      import :: c_ptr, c_int
      type(c_ptr), value :: oc, atm, tauxa, tauya, uekat, vekat, wekta, wekpa, tauxo, tauyo, wekto, wekpo, txi
    end function
    integer(c_int) function qgcm_hip_coupled_set_xforc(oc, atm, on) bind(C, name='qgcm_hip_coupled_set_xforc')
      import :: c_ptr, c_int
      type(c_ptr), value :: oc, atm
      integer(c_int), value :: on
    end function
    ! atmospheric mixed layer on the device (src/amlsubs.F); every field is a c_ptr (c_loc of the host array, or
    ! c_null_ptr to leave / skip it); diag(3*(nla-1)+2): xan(:), enisat(:), eninat(:), cfraat, centat
    integer(c_int) function qgcm_hip_aml_init(atm, prm) bind(C, name='qgcm_hip_aml_init')
      import :: c_ptr, c_int, qgcm_hip_aml_params
      type(c_ptr), value :: atm
      type(qgcm_hip_aml_params), intent(in) :: prm
    end function
    integer(c_int) function qgcm_hip_aml_set_state(atm, ast, astm, hmixa, hmixam) bind(C, name='qgcm_hip_aml_set_state')
      import :: c_ptr, c_int
      type(c_ptr), value :: atm, ast, astm, hmixa, hmixam
    end function
    integer(c_int) function qgcm_hip_aml_get_state(atm, ast, astm, hmixa, hmixam) bind(C, name='qgcm_hip_aml_get_state')
      import :: c_ptr, c_int
      type(c_ptr), value :: atm, ast, astm, hmixa, hmixam
    end function
    integer(c_int) function qgcm_hip_aml(atm) bind(C, name='qgcm_hip_aml')
      import :: c_ptr, c_int
      type(c_ptr), value :: atm
    end function
    integer(c_int) function qgcm_hip_aml_get_diag(atm, entat, diag) bind(C, name='qgcm_hip_aml_get_diag')
      import :: c_ptr, c_int
      type(c_ptr), value :: atm, entat, diag
    end function
    ! heat half of xforc on the device (src/xfosubs.F:711-853); scal: arlaav, slhfav, oradav, arocav
    integer(c_int) function qgcm_hip_xforc_heat_init(oc, atm, prm) bind(C, name='qgcm_hip_xforc_heat_init')
      import :: c_ptr, c_int, qgcm_hip_xforc_heat_params
      type(c_ptr), value :: oc, atm
      type(qgcm_hip_xforc_heat_params), intent(in) :: prm
    end function
    integer(c_int) function qgcm_hip_xforc_heat_get(oc, atm, fnetoc, fnetat, scal) bind(C, name='qgcm_hip_xforc_heat_get')
      import :: c_ptr, c_int
      type(c_ptr), value :: oc, atm, fnetoc, fnetat, scal
    end function
    ! ... without an ocean (atmos_only), from a prescribed SST held by the atmosphere handle
    integer(c_int) function qgcm_hip_xforc_sst_init(atm, prm) bind(C, name='qgcm_hip_xforc_sst_init')
      import :: c_ptr, c_int, qgcm_hip_xforc_sst_params
      type(c_ptr), value :: atm
      type(qgcm_hip_xforc_sst_params), intent(in) :: prm
    end function
    integer(c_int) function qgcm_hip_xforc_sst_set(atm, sst) bind(C, name='qgcm_hip_xforc_sst_set')
      import :: c_ptr, c_int
      type(c_ptr), value :: atm, sst
    end function
    integer(c_int) function qgcm_hip_xforc_sst_get(atm, fnetat, scal) bind(C, name='qgcm_hip_xforc_sst_get')
      import :: c_ptr, c_int
      type(c_ptr), value :: atm, fnetat, scal
    end function
  end interface

contains

  ! The reference's error convention is print + stop (e.g. src/ocisubs.F:361-365).
  ! QGCM_HIP_ABI_VERSION of include/qgcm_hip.h this interface block was written against: an older libqgcm_hip.so
  ! (without qgcm_hip_get_monitors / qgcm_hip_set_sponge, or with the other halo default) must not be driven by it
  subroutine qgcm_hip_check_abi
    integer(c_int), parameter :: want = 3
    if (qgcm_hip_abi_version() /= want) then
      print *, ' qgcm_hip: libqgcm_hip.so has ABI version ', qgcm_hip_abi_version(), ', this host binds version ', want
      print *, ' program terminates'
      stop 1
    endif
  end subroutine qgcm_hip_check_abi

  subroutine qgcm_hip_check(rc, where)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    integer :: i
    if (rc == 0) return
    call c_f_pointer(qgcm_hip_last_error(), msg, [512])
    print *, ' qgcm_hip error in ', where, ':'
    do i = 1, 512
      if (msg(i) == c_null_char) exit
      write(*, '(a)', advance='no') msg(i)
    enddo
    print *
    print *, ' program terminates'
    stop 1
  end subroutine qgcm_hip_check

end module qgcm_hip_iface
