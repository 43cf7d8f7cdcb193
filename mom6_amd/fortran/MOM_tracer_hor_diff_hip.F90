!> Drop-in replacement for module MOM_tracer_hor_diff (src/tracer/MOM_tracer_hor_diff.F90): tracer_hordiff (:119),
!! tracer_hor_diff_init (:1625) and tracer_hor_diff_end (:1772) with the reference's dummy-argument lists, so
!! step_MOM_tracer_dyn (src/core/MOM.F90:1441) compiles unchanged.  Provided: the along-layer diffusion with a constant
!! KHTR (MAX_TR_DIFFUSION_CFL, CHECK_DIFFUSIVE_CFL, the tracers' conc_underflow) or, with VarMix%use_variable_mixing, the face
!! diffusivities of :236-281 (KHTR_SLOPE_CFF with VarMix%L2u / SN_u, MEKE%KhTr_fac with MEKE%Kh, KHTR_MIN / KHTR_MAX,
!! RESOLN_SCALED_KHTR with VarMix%Res_fn_h, KHTR_PASSIVITY_COEFF / _MIN with VarMix%Rd_dx_h) on the GPU through libmom6hip
!! (mom6hip_tracer_hordiff_varmix, HOST memspace), and with USE_NEUTRAL_DIFFUSION the continuous branch of MOM_neutral_diffusion
!! (neutral_diffusion_init :138, neutral_diffusion_calc_coeffs :337, neutral_diffusion :605: NDIFF_REF_PRES, NDIFF_ANSWER_DATE,
!! RECALC_NEUTRAL_SURF, NDIFF_INTERIOR_ONLY with visc%h_ML and NDIFF_TAPERING; mom6hip_tracer_hordiff_neutral), with
!! USE_HORIZONTAL_BOUNDARY_DIFFUSION the horizontal boundary diffusion of MOM_hor_bnd_diffusion before either
!! (mom6hip_tracer_hordiff_hbd), with KHTR_USE_EBT_STRUCT the interface coefficients of both that decay with VarMix%ebt_struct
!! (FULL_DEPTH_KHTR_MIN), and with DIFFUSE_ML_TO_INTERIOR the epipycnal diffusion between the variable-density layers and the interior
!! of a layered run (tracer_epipycnal_ML_diff :700, ML_KHTR_SCALE, HOR_DIFF_ANSWER_DATE, HOR_DIFF_LIMIT_BUG;
!! mom6hip_tracer_hordiff_epipycnal).  NDIFF_CONTINUOUS = False goes to mom6hip_tracer_hordiff_neutral_discontinuous with the
!! parameters of MOM_neutral_diffusion.F90:219-277 (the interface takes hbd and ndd by reference: CS%hbd stands in where HBD is off).
!! The df_x / df_y / df2d_x / df2d_y flux diagnostics of the along-layer loop are passed on where they are associated
!! (mom6hip_tracer_hordiff_diag, mom6hip_tracer_hordiff_epipycnal_diag; left zeroed with USE_NEUTRAL_DIFFUSION).
!! NDIFF_USE_UNMASKED_TRANSPORT_BUG, offline khdt arrays, the hbd_* diagnostics, df2d_x / df2d_y with DIFFUSE_ML_TO_INTERIOR and the
!! arrays with USE_HORIZONTAL_BOUNDARY_DIFFUSION stop with a FATAL error.
!! What neutral_diffusion and hor_bnd_diffusion post themselves is posted here: with USE_NEUTRAL_DIFFUSION a tracer's id_dfx_2d, id_dfy_2d,
!! id_dfxy_cont, id_dfxy_cont_2d and id_dfxy_conc, and, where USE_NEUTRAL_DIFFUSION follows USE_HORIZONTAL_BOUNDARY_DIFFUSION, its
!! id_hbd_dfx, id_hbd_dfy, id_hbd_dfx_2d, id_hbd_dfy_2d, id_hbdxy_cont, id_hbdxy_cont_2d and id_hbdxy_conc get a zero-filled work array
!! each (the reference's posted arrays are zero outside the compute range), mom6hip_tracer_hordiff_mix_diag fills their compute ranges,
!! and post_data is called in the reference's order (the boundary diffusion's posts tracer after tracer, then neutral diffusion's).
!! Still refused: an hbd_* id with the boundary diffusion followed by the along-layer loop (FATAL here), and any of these ids with
!! more than one iteration (MAX_TR_DIFFUSION_CFL, CHECK_DIFFUSIVE_CFL): the library's refusal is passed on as FATAL.
!!
!! Compiled INSIDE a MOM6 source tree in place of src/tracer/MOM_tracer_hor_diff.F90; here against tests/fortran/stubs.
module MOM_tracer_hor_diff

use, intrinsic :: iso_c_binding
use mom6hip_c_api
use mom6hip_MOM_glue,          only : mom6hip_shared_context, mom6hip_read_topology, mom6hip_fatal_if
use mom6hip_MOM_glue,          only : mom6hip_read_resident, mom6hip_resident, mom6hip_mirror, mom6hip_read_eos, mom6hip_mirror_to_host
use MOM_cpu_clock,             only : cpu_clock_id, cpu_clock_begin, cpu_clock_end, CLOCK_MODULE
use MOM_CVMix_KPP,             only : KPP_CS
use MOM_diabatic_driver,       only : diabatic_CS, extract_diabatic_member
use MOM_energetic_PBL,         only : energetic_PBL_CS
use MOM_diag_mediator,         only : diag_ctrl, time_type, post_data
use MOM_EOS,                   only : EOS_type
use MOM_error_handler,         only : MOM_error, FATAL, WARNING
use MOM_file_parser,           only : get_param, log_version, param_file_type
use MOM_grid,                  only : ocean_grid_type
use MOM_lateral_mixing_coeffs, only : VarMix_CS
use MOM_MEKE_types,            only : MEKE_type
use MOM_tracer_registry,       only : tracer_registry_type
use MOM_unit_scaling,          only : unit_scale_type
use MOM_variables,             only : thermo_var_ptrs, vertvisc_type
use MOM_verticalGrid,          only : verticalGrid_type
implicit none ; private

#include <MOM_memory.h>

public tracer_hordiff, tracer_hor_diff_init, tracer_hor_diff_end

!> Control structure (the members of the reference's tracer_hor_diff_CS, :40-100, that the provided branch reads)
type, public :: tracer_hor_diff_CS ; private
  real    :: KhTr                 !< The along-isopycnal tracer diffusivity [L2 T-1 ~> m2 s-1].
  real    :: KhTr_Slope_Cff       !< The non-dimensional coefficient in KhTr formula [nondim]
  real    :: KhTr_min             !< Minimum along-isopycnal tracer diffusivity [L2 T-1 ~> m2 s-1].
  real    :: KhTr_max             !< Maximum along-isopycnal tracer diffusivity [L2 T-1 ~> m2 s-1].
  real    :: KhTr_passivity_coeff !< Passivity coefficient that scales Rd/dx [nondim]
  real    :: KhTr_passivity_min   !< Passivity minimum [nondim]
  real    :: max_diff_CFL         !< If positive, locally limit the diffusivity to this diffusive CFL [nondim].
  logical :: check_diffusive_CFL  !< If true, use enough iterations that the diffusive equations are stable.
  logical :: KhTr_use_ebt_struct  !< If true, uses the equivalent barotropic structure as the vertical structure of the diffusivity.
  logical :: full_depth_khtr_min  !< If true, KHTR_MIN is enforced throughout the whole water column.
  logical :: Diffuse_ML_interior, use_neutral_diffusion, use_hor_bnd_diffusion
  logical :: first_call = .true.
  logical :: recalc_neutral_surf  !< If true, recalculate the neutral surfaces if CFL has been exceeded
  type(mom6hip_neutral_diffusion_cs_t) :: nd   !< neutral_diffusion_CS as the library reads it
  type(mom6hip_ndiff_discontinuous_cs_t) :: ndd !< its parameters of NDIFF_CONTINUOUS = False (MOM_neutral_diffusion.F90:219-277)
  type(mom6hip_epipycnal_cs_t) :: epi          !< the parameters of tracer_epipycnal_ML_diff as the library reads them
  type(mom6hip_hor_bnd_diffusion_cs_t) :: hbd  !< hbd_CS (USE_HORIZONTAL_BOUNDARY_DIFFUSION) as the library reads it
  type(mom6hip_eos_t) :: eos                   !< the equation of state tracer_hor_diff_init was given
  type(diag_ctrl), pointer :: diag => NULL()
end type tracer_hor_diff_CS

integer :: id_clock_diffuse

contains

!> Same interface as the reference tracer_hordiff (:119).
subroutine tracer_hordiff(h, dt, MEKE, VarMix, visc, G, GV, US, CS, Reg, tv, do_online_flag, read_khdt_x, read_khdt_y)
  type(ocean_grid_type),      intent(inout) :: G
  type(verticalGrid_type),    intent(in)    :: GV
  real, dimension(SZI_(G),SZJ_(G),SZK_(GV)), target, intent(in) :: h
  real,                       intent(in)    :: dt
  type(MEKE_type), target,    intent(in)    :: MEKE
  type(VarMix_CS), target,    intent(in)    :: VarMix
  type(vertvisc_type),        intent(in)    :: visc
  type(unit_scale_type),      intent(in)    :: US
  type(tracer_hor_diff_CS),   pointer       :: CS
  type(tracer_registry_type), pointer       :: Reg
  type(thermo_var_ptrs),      intent(in)    :: tv
  logical,          optional, intent(in)    :: do_online_flag
  real, dimension(SZIB_(G),SZJ_(G)), optional, intent(in) :: read_khdt_x
  real, dimension(SZI_(G),SZJB_(G)), optional, intent(in) :: read_khdt_y

  type(mom6hip_tracer_hor_diff_cs_t) :: ccs
  type(mom6hip_hordiff_fields_t) :: fld
  type(c_ptr) :: ctx
  type(mom6hip_hordiff_stats_t) :: stats
  type(c_ptr), allocatable :: tr(:)
  real(c_double), allocatable, target :: cu(:)
  type(c_ptr) :: p_surf
  real(c_double), allocatable, target :: Rlay(:)
  integer :: m, rc, idx_T, idx_S, q, k
  logical :: any_diag
  type(mom6hip_tracer_flux_diag_t), allocatable, target :: dg(:)      ! the device (resident) or host (staged) arrays of the call
  type(c_ptr), allocatable :: dgh(:,:)                                ! the host arrays behind them
  type(c_ptr) :: p_dg
  ! what neutral_diffusion and hor_bnd_diffusion post themselves (mom6hip_tracer_mix_diag_t): the work arrays of the call are slices of
  ! one zero-filled host block (and, resident, of one zeroed device block that is copied back before the posts)
  type(mom6hip_tracer_mix_diag_t), allocatable, target :: mx(:)
  real(c_double), allocatable, target :: pool(:)
  integer(c_int64_t), allocatable :: mix_off(:,:)      ! (12, ntr): the offset of an array in the block, -1: not asked for
  integer(c_int64_t) :: mix_n(12), mix_tot, nu2, nv2, nh2
  integer :: mix_id(12)
  logical :: any_mix
  type(c_ptr) :: d_pool, p_ndd

  if (.not. associated(CS)) call MOM_error(FATAL, "MOM_tracer_hor_diff: "// &
       "register_tracer must be called before tracer_hordiff.")
  if (.not. associated(Reg)) call MOM_error(FATAL, "MOM_tracer_hor_diff: "// &
       "register_tracer must be called before tracer_hordiff.")
  if (Reg%ntr == 0 .or. (CS%KhTr <= 0.0 .and. .not. VarMix%use_variable_mixing)) return
  if (present(do_online_flag)) then ; if (.not.do_online_flag) &
    call MOM_error(FATAL, "tracer_hordiff (HIP): offline tracer diffusion (read_khdt_x/y) is not provided by the GPU path.")
  endif
  call cpu_clock_begin(id_clock_diffuse)
  CS%first_call = .false.

  allocate(tr(Reg%ntr), cu(Reg%ntr))
  do m=1,Reg%ntr
    if (CS%use_hor_bnd_diffusion .and. .not.CS%use_neutral_diffusion .and. (Reg%Tr(m)%id_hbdxy_cont > 0 .or. Reg%Tr(m)%id_hbdxy_cont_2d > 0 .or. &
        Reg%Tr(m)%id_hbdxy_conc > 0 .or. Reg%Tr(m)%id_hbd_dfx > 0 .or. Reg%Tr(m)%id_hbd_dfy > 0 .or. Reg%Tr(m)%id_hbd_dfx_2d > 0 .or. &
        Reg%Tr(m)%id_hbd_dfy_2d > 0)) call MOM_error(FATAL, "tracer_hordiff (HIP): the hbd_* diagnostics of tracer "// &
        trim(Reg%Tr(m)%name)//" are not provided by the GPU path.")
    tr(m) = c_loc(Reg%Tr(m)%t)
    cu(m) = Reg%Tr(m)%conc_underflow
  enddo
  ! the diffusive flux diagnostics where they are associated (:389-406, :576-591)
  allocate(dg(Reg%ntr), dgh(4,Reg%ntr)) ; any_diag = .false. ; dgh(:,:) = c_null_ptr
  do m=1,Reg%ntr
    if (associated(Reg%Tr(m)%df_x)) dgh(1,m) = c_loc(Reg%Tr(m)%df_x)
    if (associated(Reg%Tr(m)%df_y)) dgh(2,m) = c_loc(Reg%Tr(m)%df_y)
    if (associated(Reg%Tr(m)%df2d_x)) dgh(3,m) = c_loc(Reg%Tr(m)%df2d_x)
    if (associated(Reg%Tr(m)%df2d_y)) dgh(4,m) = c_loc(Reg%Tr(m)%df2d_y)
    do q=1,4 ; if (c_associated(dgh(q,m))) any_diag = .true. ; enddo
    dg(m)%df_x = dgh(1,m) ; dg(m)%df_y = dgh(2,m) ; dg(m)%df2d_x = dgh(3,m) ; dg(m)%df2d_y = dgh(4,m)
  enddo
  if (any_diag .and. CS%use_neutral_diffusion) then
    ! the along-layer loop does not run: the arrays stay as the reference zeroes them (:389-406), on the host where they are read
    do m=1,Reg%ntr
      if (associated(Reg%Tr(m)%df_x)) then ; do k=1,GV%ke
        Reg%Tr(m)%df_x(G%isc-1:G%iec,G%jsc:G%jec,k) = 0.0
      enddo ; endif
      if (associated(Reg%Tr(m)%df_y)) then ; do k=1,GV%ke
        Reg%Tr(m)%df_y(G%isc:G%iec,G%jsc-1:G%jec,k) = 0.0
      enddo ; endif
      if (associated(Reg%Tr(m)%df2d_x)) Reg%Tr(m)%df2d_x(G%isc-1:G%iec,G%jsc:G%jec) = 0.0
      if (associated(Reg%Tr(m)%df2d_y)) Reg%Tr(m)%df2d_y(G%isc:G%iec,G%jsc-1:G%jec) = 0.0
    enddo
    any_diag = .false.
  endif
  if (any_diag .and. CS%use_hor_bnd_diffusion) call MOM_error(FATAL, "tracer_hordiff (HIP): the diffusive flux diagnostics (df_x, df_y, "// &
      "df2d_x, df2d_y) together with USE_HORIZONTAL_BOUNDARY_DIFFUSION and the along-layer diffusion are not provided by the GPU path.")
  p_dg = c_null_ptr ; if (any_diag) p_dg = c_loc(dg)
  ! the ids of the posts of neutral_diffusion (MOM_neutral_diffusion.F90:935-1014) and, where it follows the boundary diffusion, of
  ! hor_bnd_diffusion (MOM_hor_bnd_diffusion.F90:292-333), in the order of the record
  nu2 = int(size(h,1)+1, c_int64_t) * size(h,2) ; nv2 = int(size(h,1), c_int64_t) * (size(h,2)+1) ; nh2 = int(size(h,1), c_int64_t) * size(h,2)
  mix_n(:) = (/ nu2, nv2, nh2*GV%ke, nh2, nh2*GV%ke, nu2*GV%ke, nv2*GV%ke, nu2, nv2, nh2*GV%ke, nh2, nh2*GV%ke /)
  allocate(mix_off(12,Reg%ntr), mx(Reg%ntr)) ; mix_off(:,:) = -1 ; mix_tot = 0 ; any_mix = .false.
  if (CS%use_neutral_diffusion) then ; do m=1,Reg%ntr
    call mix_ids(m)
    do q=1,12 ; if (mix_id(q) > 0 .and. (q <= 5 .or. CS%use_hor_bnd_diffusion)) then
      mix_off(q,m) = mix_tot ; mix_tot = mix_tot + mix_n(q) ; any_mix = .true.
    endif ; enddo
  enddo ; endif
  if (any_mix) then
    allocate(pool(mix_tot)) ; pool(:) = 0.0
    if (.not.mom6hip_resident()) then
      do m=1,Reg%ntr ; do q=1,12 ; if (mix_off(q,m) >= 0) call mix_set(mx(m), q, c_loc(pool(mix_off(q,m)+1))) ; enddo ; enddo
    endif
    p_ndd = c_null_ptr ; if (CS%nd%unsupported(1) /= 0) p_ndd = c_loc(CS%ndd)
  endif
  ccs%KhTr = CS%KhTr ; ccs%max_diff_CFL = CS%max_diff_CFL
  ccs%KhTr_Slope_Cff = CS%KhTr_Slope_Cff ; ccs%KhTr_min = CS%KhTr_min ; ccs%KhTr_max = CS%KhTr_max
  ccs%KhTr_passivity_coeff = CS%KhTr_passivity_coeff ; ccs%KhTr_passivity_min = CS%KhTr_passivity_min
  ccs%check_diffusive_CFL = merge(1, 0, CS%check_diffusive_CFL) ; ccs%initialized = 1
  ccs%unsupported(:) = 0 ; ccs%reserved1(:) = 0 ; ccs%full_depth_khtr_min = merge(1, 0, CS%full_depth_khtr_min)
  if (CS%KhTr_use_ebt_struct) then      ! :428-462, :503-518
    ccs%unsupported(6) = 1
    if (CS%use_neutral_diffusion .or. CS%use_hor_bnd_diffusion) then
      if (.not.allocated(VarMix%ebt_struct)) call MOM_error(FATAL, "tracer_hordiff (HIP): KHTR_USE_EBT_STRUCT needs VarMix%ebt_struct.")
      fld%ebt_struct = c_loc(VarMix%ebt_struct)
    endif
  endif
  if (VarMix%use_variable_mixing) then      ! :219-224, :236-281
    ccs%use_variable_mixing = 1
    if (CS%KhTr_Slope_Cff > 0.) then
      fld%L2u = c_loc(VarMix%L2u) ; fld%L2v = c_loc(VarMix%L2v) ; fld%SN_u = c_loc(VarMix%SN_u) ; fld%SN_v = c_loc(VarMix%SN_v)
    endif
    if (VarMix%Resoln_scaled_KhTr) then ; ccs%Resoln_scaled_KhTr = 1 ; fld%Res_fn_h = c_loc(VarMix%Res_fn_h) ; endif
    if (CS%KhTr_passivity_coeff > 0.) fld%Rd_dx_h = c_loc(VarMix%Rd_dx_h)
    if (allocated(MEKE%Kh)) then ; fld%MEKE_Kh = c_loc(MEKE%Kh) ; ccs%KhTr_fac = MEKE%KhTr_fac ; endif
  endif
  idx_T = -1 ; idx_S = -1 ; p_surf = c_null_ptr
  if (CS%use_neutral_diffusion) then      ! :474-534: tv%T and tv%S are registered tracers, found by association
    ccs%unsupported(1) = 1
    if (.not.(associated(tv%T) .and. associated(tv%S))) call MOM_error(FATAL, &
      "tracer_hordiff (HIP): USE_NEUTRAL_DIFFUSION needs tv%T and tv%S.")
    do m=1,Reg%ntr
      if (associated(Reg%Tr(m)%t, tv%T)) idx_T = m-1
      if (associated(Reg%Tr(m)%t, tv%S)) idx_S = m-1
    enddo
    if (idx_T < 0 .or. idx_S < 0) call MOM_error(FATAL, "tracer_hordiff (HIP): tv%T and tv%S must be registered tracers.")
    if (associated(tv%p_surf)) p_surf = c_loc(tv%p_surf)
    if (CS%nd%interior_only /= 0) then      ! MOM_neutral_diffusion.F90:372-378
      if (.not.associated(visc%h_ML)) call MOM_error(FATAL, "hor_bnd_diffusion requires that visc%h_ML is associated.")
      fld%h_ML = c_loc(visc%h_ML)
    endif
    CS%nd%H_to_RZ = GV%H_to_RZ ; CS%nd%recalc_neutral_surf = merge(1, 0, CS%recalc_neutral_surf)
  endif
  if (CS%use_hor_bnd_diffusion) then      ! :408-472, hor_bnd_diffusion :217-221
    ccs%unsupported(2) = 1
    if (.not.associated(visc%h_ML)) call MOM_error(FATAL, "hor_bnd_diffusion requires that visc%h_ML is associated.")
    fld%h_ML = c_loc(visc%h_ML)
  endif
  if (CS%Diffuse_ML_interior) then      ! :544-550, :613-620: tv%T and tv%S are registered tracers, found by association
    ccs%unsupported(3) = 1
    if (.not.(associated(tv%T) .and. associated(tv%S))) call MOM_error(FATAL, &
      "tracer_hordiff (HIP): DIFFUSE_ML_TO_INTERIOR needs tv%T and tv%S.")
    do m=1,Reg%ntr
      if (associated(Reg%Tr(m)%t, tv%T)) idx_T = m-1
      if (associated(Reg%Tr(m)%t, tv%S)) idx_S = m-1
    enddo
    if (idx_T < 0 .or. idx_S < 0) call MOM_error(FATAL, "tracer_hordiff (HIP): tv%T and tv%S must be registered tracers.")
    allocate(Rlay(GV%ke)) ; Rlay(:) = GV%Rlay(1:GV%ke)
    CS%epi%Rlay = c_loc(Rlay) ; CS%epi%nkml = GV%nkml ; CS%epi%nk_rho_varies = GV%nk_rho_varies ; CS%epi%P_Ref = tv%P_Ref
  endif
  if (mom6hip_resident()) then      ! GPU_RESIDENT_DYNAMICS: the shared device mirrors of the host arrays
    ctx = mom6hip_shared_context(G, GV)
    do m=1,Reg%ntr ; tr(m) = mom6hip_mirror(ctx, tr(m), int(size(h), c_int64_t), .true., .true.) ; enddo
    call to_dev(p_surf, size(h(:,:,1))) ; call to_dev(fld%h_ML, size(h(:,:,1))) ; call to_dev(fld%ebt_struct, size(h))
    call to_dev(fld%MEKE_Kh, size(h(:,:,1))) ; call to_dev(fld%Res_fn_h, size(h(:,:,1))) ; call to_dev(fld%Rd_dx_h, size(h(:,:,1)))
    if (c_associated(fld%L2u)) then
      call to_dev(fld%L2u, size(VarMix%L2u)) ; call to_dev(fld%SN_u, size(VarMix%SN_u))
      call to_dev(fld%L2v, size(VarMix%L2v)) ; call to_dev(fld%SN_v, size(VarMix%SN_v))
    endif
    if (any_diag) then      ! the call writes a range of each array: mirrors that are read and written
      do m=1,Reg%ntr
        if (c_associated(dgh(1,m))) dg(m)%df_x = mom6hip_mirror(ctx, dgh(1,m), int(size(Reg%Tr(m)%df_x), c_int64_t), .true., .true.)
        if (c_associated(dgh(2,m))) dg(m)%df_y = mom6hip_mirror(ctx, dgh(2,m), int(size(Reg%Tr(m)%df_y), c_int64_t), .true., .true.)
        if (c_associated(dgh(3,m))) dg(m)%df2d_x = mom6hip_mirror(ctx, dgh(3,m), int(size(Reg%Tr(m)%df2d_x), c_int64_t), .true., .true.)
        if (c_associated(dgh(4,m))) dg(m)%df2d_y = mom6hip_mirror(ctx, dgh(4,m), int(size(Reg%Tr(m)%df2d_y), c_int64_t), .true., .true.)
      enddo
    endif
    if (any_mix) then
      rc = mom6hip_malloc(d_pool, 8_c_int64_t*mix_tot) ; call mom6hip_fatal_if(rc, "tracer_hordiff")
      rc = mom6hip_memset_zero(ctx, d_pool, 8_c_int64_t*mix_tot) ; call mom6hip_fatal_if(rc, "tracer_hordiff")
      do m=1,Reg%ntr ; do q=1,12 ; if (mix_off(q,m) >= 0) &
        call mix_set(mx(m), q, transfer(transfer(d_pool, 0_c_intptr_t) + 8_c_intptr_t*mix_off(q,m), d_pool)) ; enddo ; enddo
      rc = mom6hip_tracer_hordiff_mix_diag(ctx, ccs, merge(c_loc(CS%hbd), c_null_ptr, CS%use_hor_bnd_diffusion), c_loc(CS%nd), p_ndd, fld, &
                                      mom6hip_mirror(ctx, c_loc(h), int(size(h), c_int64_t), .true., .false.), c_loc(CS%eos), p_surf, dt, tr, &
                                      c_loc(cu), int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), int(idx_S, c_int32_t), MOM6HIP_MEM_DEVICE, &
                                      stats, c_loc(mx))
      if (rc == 0) rc = mom6hip_sync_to_host(ctx, c_loc(pool), d_pool, 8_c_int64_t*mix_tot)
      q = mom6hip_free(d_pool)
    elseif (CS%Diffuse_ML_interior) then
      rc = mom6hip_tracer_hordiff_epipycnal_diag(ctx, ccs, CS%epi, fld, mom6hip_mirror(ctx, c_loc(h), int(size(h), c_int64_t), .true., .false.), &
                                            CS%eos, dt, tr, c_loc(cu), int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), &
                                            int(idx_S, c_int32_t), MOM6HIP_MEM_DEVICE, stats, p_dg)
    elseif (any_diag) then
      rc = mom6hip_tracer_hordiff_diag(ctx, ccs, fld, mom6hip_mirror(ctx, c_loc(h), int(size(h), c_int64_t), .true., .false.), dt, tr, &
                                       c_loc(cu), int(Reg%ntr, c_int32_t), MOM6HIP_MEM_DEVICE, stats, p_dg)
    elseif (CS%use_neutral_diffusion .and. CS%nd%unsupported(1) /= 0) then      ! NDIFF_CONTINUOUS = False (CS%hbd is read with HBD only)
      rc = mom6hip_tracer_hordiff_neutral_discontinuous(ctx, ccs, CS%hbd, CS%nd, CS%ndd, fld, &
                                      mom6hip_mirror(ctx, c_loc(h), int(size(h), c_int64_t), .true., .false.), &
                                      CS%eos, p_surf, dt, tr, c_loc(cu), int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), &
                                      int(idx_S, c_int32_t), MOM6HIP_MEM_DEVICE, stats)
    elseif (CS%use_hor_bnd_diffusion) then
      rc = mom6hip_tracer_hordiff_hbd(ctx, ccs, CS%hbd, CS%nd, fld, mom6hip_mirror(ctx, c_loc(h), int(size(h), c_int64_t), .true., .false.), &
                                      CS%eos, p_surf, dt, tr, c_loc(cu), int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), &
                                      int(idx_S, c_int32_t), MOM6HIP_MEM_DEVICE, stats)
    else
    rc = mom6hip_tracer_hordiff_neutral(ctx, ccs, CS%nd, fld, mom6hip_mirror(ctx, c_loc(h), int(size(h), c_int64_t), .true., .false.), &
                                        CS%eos, p_surf, dt, tr, c_loc(cu), int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), &
                                        int(idx_S, c_int32_t), MOM6HIP_MEM_DEVICE, stats)
    endif
  elseif (any_mix) then
    rc = mom6hip_tracer_hordiff_mix_diag(mom6hip_shared_context(G, GV), ccs, merge(c_loc(CS%hbd), c_null_ptr, CS%use_hor_bnd_diffusion), &
                                    c_loc(CS%nd), p_ndd, fld, c_loc(h), c_loc(CS%eos), p_surf, dt, tr, c_loc(cu), int(Reg%ntr, c_int32_t), &
                                    int(idx_T, c_int32_t), int(idx_S, c_int32_t), MOM6HIP_MEM_HOST, stats, c_loc(mx))
  elseif (CS%Diffuse_ML_interior) then
    rc = mom6hip_tracer_hordiff_epipycnal_diag(mom6hip_shared_context(G, GV), ccs, CS%epi, fld, c_loc(h), CS%eos, dt, tr, c_loc(cu), &
                                          int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), int(idx_S, c_int32_t), MOM6HIP_MEM_HOST, stats, p_dg)
  elseif (any_diag) then
    rc = mom6hip_tracer_hordiff_diag(mom6hip_shared_context(G, GV), ccs, fld, c_loc(h), dt, tr, c_loc(cu), int(Reg%ntr, c_int32_t), &
                                     MOM6HIP_MEM_HOST, stats, p_dg)
  elseif (CS%use_neutral_diffusion .and. CS%nd%unsupported(1) /= 0) then
    rc = mom6hip_tracer_hordiff_neutral_discontinuous(mom6hip_shared_context(G, GV), ccs, CS%hbd, CS%nd, CS%ndd, fld, c_loc(h), CS%eos, &
                                    p_surf, dt, tr, c_loc(cu), int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), int(idx_S, c_int32_t), &
                                    MOM6HIP_MEM_HOST, stats)
  elseif (CS%use_hor_bnd_diffusion) then
    rc = mom6hip_tracer_hordiff_hbd(mom6hip_shared_context(G, GV), ccs, CS%hbd, CS%nd, fld, c_loc(h), CS%eos, p_surf, dt, tr, c_loc(cu), &
                                    int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), int(idx_S, c_int32_t), MOM6HIP_MEM_HOST, stats)
  else
    rc = mom6hip_tracer_hordiff_neutral(mom6hip_shared_context(G, GV), ccs, CS%nd, fld, c_loc(h), CS%eos, p_surf, dt, tr, c_loc(cu), &
                                        int(Reg%ntr, c_int32_t), int(idx_T, c_int32_t), int(idx_S, c_int32_t), MOM6HIP_MEM_HOST, stats)
  endif
  CS%epi%Rlay = c_null_ptr
  call mom6hip_fatal_if(rc, "tracer_hordiff")
  ! the host posts the arrays right after this call
  if (any_diag .and. mom6hip_resident()) then
    do m=1,Reg%ntr ; do q=1,4 ; if (c_associated(dgh(q,m))) call mom6hip_mirror_to_host(ctx, dgh(q,m)) ; enddo ; enddo
  endif
  ! the posts, in the reference's order: hor_bnd_diffusion's tracer after tracer (it runs first), then neutral_diffusion's
  if (any_mix) then
    do m=1,Reg%ntr ; call mix_ids(m) ; do q=6,12 ; if (mix_off(q,m) >= 0) call mix_post(q, mix_id(q), mix_off(q,m)) ; enddo ; enddo
    do m=1,Reg%ntr ; call mix_ids(m) ; do q=1,5 ; if (mix_off(q,m) >= 0) call mix_post(q, mix_id(q), mix_off(q,m)) ; enddo ; enddo
  endif
  call cpu_clock_end(id_clock_diffuse)
contains
  !> the twelve diagnostic ids of tracer m, in the order of mom6hip_tracer_mix_diag_t
  subroutine mix_ids(m)
    integer, intent(in) :: m
    mix_id(:) = (/ Reg%Tr(m)%id_dfx_2d, Reg%Tr(m)%id_dfy_2d, Reg%Tr(m)%id_dfxy_cont, Reg%Tr(m)%id_dfxy_cont_2d, Reg%Tr(m)%id_dfxy_conc, &
                   Reg%Tr(m)%id_hbd_dfx, Reg%Tr(m)%id_hbd_dfy, Reg%Tr(m)%id_hbd_dfx_2d, Reg%Tr(m)%id_hbd_dfy_2d, Reg%Tr(m)%id_hbdxy_cont, &
                   Reg%Tr(m)%id_hbdxy_cont_2d, Reg%Tr(m)%id_hbdxy_conc /)
  end subroutine mix_ids
  !> member q of a record
  subroutine mix_set(r, q, p)
    type(mom6hip_tracer_mix_diag_t), intent(inout) :: r
    integer,     intent(in) :: q
    type(c_ptr), intent(in) :: p
    select case (q)
      case (1) ; r%dfx_2d = p ; case (2) ; r%dfy_2d = p ; case (3) ; r%dfxy_cont = p ; case (4) ; r%dfxy_cont_2d = p
      case (5) ; r%dfxy_conc = p ; case (6) ; r%hbd_dfx = p ; case (7) ; r%hbd_dfy = p ; case (8) ; r%hbd_dfx_2d = p
      case (9) ; r%hbd_dfy_2d = p ; case (10) ; r%hbdxy_cont = p ; case (11) ; r%hbdxy_cont_2d = p ; case (12) ; r%hbdxy_conc = p
    end select
  end subroutine mix_set
  !> post_data of the array q at offset off of the host block, with the bounds of the reference's local array
  subroutine mix_post(q, id, off)
    integer,            intent(in) :: q, id
    integer(c_int64_t), intent(in) :: off
    real, pointer :: a2(:,:), a3(:,:,:)
    select case (q)
      case (1, 8) ; a2(G%IsdB:G%IedB,G%jsd:G%jed) => pool(off+1:off+mix_n(q))
      case (2, 9) ; a2(G%isd:G%ied,G%JsdB:G%JedB) => pool(off+1:off+mix_n(q))
      case (4, 11) ; a2(G%isd:G%ied,G%jsd:G%jed) => pool(off+1:off+mix_n(q))
      case (6) ; a3(G%IsdB:G%IedB,G%jsd:G%jed,1:GV%ke) => pool(off+1:off+mix_n(q))
      case (7) ; a3(G%isd:G%ied,G%JsdB:G%JedB,1:GV%ke) => pool(off+1:off+mix_n(q))
      case default ; a3(G%isd:G%ied,G%jsd:G%jed,1:GV%ke) => pool(off+1:off+mix_n(q))
    end select
    select case (q)
      case (1, 2, 4, 8, 9, 11) ; call post_data(id, a2, CS%diag)
      case default ; call post_data(id, a3, CS%diag)
    end select
  end subroutine mix_post
  !> a host pointer of the struct -> its device mirror (an input)
  subroutine to_dev(p, n)
    type(c_ptr), intent(inout) :: p
    integer,     intent(in)    :: n
    if (c_associated(p)) p = mom6hip_mirror(ctx, p, int(n, c_int64_t), .true., .false.)
  end subroutine to_dev
end subroutine tracer_hordiff

!> Same interface as the reference tracer_hor_diff_init (:1625), same parameters and defaults (:1652-1700).
subroutine tracer_hor_diff_init(Time, G, GV, US, param_file, diag, EOS, diabatic_CSp, CS)
  type(time_type), target,    intent(in)    :: Time
  type(ocean_grid_type),      intent(in)    :: G
  type(verticalGrid_type),    intent(in)    :: GV
  type(unit_scale_type),      intent(in)    :: US
  type(diag_ctrl), target,    intent(inout) :: diag
  type(EOS_type),  target,    intent(in)    :: EOS
  type(diabatic_CS), pointer, intent(in)    :: diabatic_CSp
  type(param_file_type),      intent(in)    :: param_file
  type(tracer_hor_diff_CS),   pointer       :: CS
# include "version_variable.h"
  character(len=40)  :: mdl = "MOM_tracer_hor_diff"
  logical :: flag

  if (associated(CS)) then
    call MOM_error(WARNING, "tracer_hor_diff_init called with associated control structure.")
    return
  endif
  allocate(CS)
  CS%diag => diag
  call log_version(param_file, mdl, version, "")
  call get_param(param_file, mdl, "KHTR", CS%KhTr, "The background along-isopycnal tracer diffusivity.", &
                 units="m2 s-1", default=0.0, scale=US%m_to_L**2*US%T_to_s)
  call get_param(param_file, mdl, "KHTR_USE_EBT_STRUCT", CS%KhTr_use_ebt_struct, &
                 "If true, uses the equivalent barotropic structure as the vertical structure of the tracer diffusivity.", &
                 default=.false.)
  call get_param(param_file, mdl, "KHTR_SLOPE_CFF", CS%KhTr_Slope_Cff, &
                 "The scaling coefficient for along-isopycnal tracer diffusivity using a shear-based (Visbeck-like) "//&
                 "parameterization.  A non-zero value enables this param.", units="nondim", default=0.0)
  call get_param(param_file, mdl, "KHTR_MIN", CS%KhTr_Min, "The minimum along-isopycnal tracer diffusivity.", &
                 units="m2 s-1", default=0.0, scale=US%m_to_L**2*US%T_to_s)
  CS%full_depth_khtr_min = .false.
  if (CS%KhTr_use_ebt_struct .and. CS%KhTr_Min > 0.0) then
    call get_param(param_file, mdl, "FULL_DEPTH_KHTR_MIN", CS%full_depth_khtr_min, &
                   "If true, KHTR_MIN is enforced throughout the whole water column. Otherwise, KHTR_MIN is only enforced at the "//&
                   "surface. This parameter is only available when KHTR_USE_EBT_STRUCT=True and KHTR_MIN>0.", default=.false.)
  endif
  call get_param(param_file, mdl, "KHTR_MAX", CS%KhTr_Max, "The maximum along-isopycnal tracer diffusivity.", &
                 units="m2 s-1", default=0.0, scale=US%m_to_L**2*US%T_to_s)
  call get_param(param_file, mdl, "KHTR_PASSIVITY_COEFF", CS%KhTr_passivity_coeff, &
                 "The coefficient that scales deformation radius over grid-spacing in passivity.", units="nondim", default=0.0)
  call get_param(param_file, mdl, "KHTR_PASSIVITY_MIN", CS%KhTr_passivity_min, &
                 "The minimum passivity which is the ratio between along isopycnal mixing of tracers to thickness mixing.", &
                 units="nondim", default=0.5)
  call get_param(param_file, mdl, "DIFFUSE_ML_TO_INTERIOR", CS%Diffuse_ML_interior, &
                 "If true, enable epipycnal mixing between the surface boundary layer and the interior.", default=.false.)
  call get_param(param_file, mdl, "CHECK_DIFFUSIVE_CFL", CS%check_diffusive_CFL, &
                 "If true, use enough iterations the diffusion to ensure that the diffusive equations are stable.", &
                 default=.false.)
  call get_param(param_file, mdl, "MAX_TR_DIFFUSION_CFL", CS%max_diff_CFL, &
                 "If positive, locally limit the along-isopycnal tracer diffusivity to keep the diffusive CFL below this.", &
                 units="nondim", default=-1.0)
  call get_param(param_file, mdl, "RECALC_NEUTRAL_SURF", CS%recalc_neutral_surf, &
                 "If true, then recalculate the neutral surfaces if the CFL has been exceeded", default=.false.)
  call get_param(param_file, mdl, "HOR_DIFF_ANSWER_DATE", CS%epi%answer_date, &
                 "The vintage of the order of arithmetic to use for the tracer diffusion.", default=20240101, &
                 do_not_log=.not.CS%Diffuse_ML_interior)
  call get_param(param_file, mdl, "HOR_DIFF_LIMIT_BUG", flag, &
                 "If true and the answer date is 20240330 or below, use a rotational symmetry breaking bug when limiting the "//&
                 "tracer properties in tracer_epipycnal_ML_diff.", default=.true., &
                 do_not_log=((.not.CS%Diffuse_ML_interior).or.(CS%epi%answer_date>=20240331)))
  CS%epi%limit_bug = merge(1, 0, flag)
  CS%epi%ML_KhTr_scale = 1.0
  if (CS%Diffuse_ML_interior) then
    call get_param(param_file, mdl, "ML_KHTR_SCALE", CS%epi%ML_KhTr_scale, &
                 "With Diffuse_ML_interior, the ratio of the truly horizontal diffusivity in the mixed layer to the "//&
                 "epipycnal diffusivity.  The valid range is 0 to 1.", units="nondim", default=1.0)
    if (GV%nk_rho_varies < 1 .or. GV%nk_rho_varies >= GV%ke) call MOM_error(FATAL, "tracer_hor_diff_init (HIP): "// &
      "DIFFUSE_ML_TO_INTERIOR is provided for layered runs with variable-density layers above an interior (0 < nk_rho_varies < nk).")
    call mom6hip_read_eos(param_file, CS%eos, "tracer_hor_diff_init")
  endif
  ! neutral_diffusion_init :138-330
  call get_param(param_file, "MOM_neutral_diffusion", "USE_NEUTRAL_DIFFUSION", CS%use_neutral_diffusion, &
                 "If true, enables the neutral diffusion module.", default=.false.)
  if (CS%use_neutral_diffusion) then
    call get_param(param_file, "MOM_neutral_diffusion", "NDIFF_CONTINUOUS", flag, &
                   "If true, uses a continuous reconstruction of T and S when finding neutral surfaces.", default=.true.)
    CS%nd%unsupported(1) = merge(0, 1, flag)      ! .not.CS%continuous_reconstruction
    call get_param(param_file, "MOM_neutral_diffusion", "NDIFF_REF_PRES", CS%nd%ref_pres, &
                   "The reference pressure (Pa) used for the derivatives of the equation of state. If negative (default), "//&
                   "local pressure is used.", units="Pa", default=-1., scale=US%Pa_to_RL2_T2)
    call get_param(param_file, "MOM_neutral_diffusion", "NDIFF_INTERIOR_ONLY", flag, &
                   "If true, only applies neutral diffusion in the ocean interior. That is, the algorithm will exclude the "//&
                   "surface and bottom boundary layers.", default=.false.)
    CS%nd%interior_only = merge(1, 0, flag)
    if (flag) then
      call get_param(param_file, "MOM_neutral_diffusion", "NDIFF_TAPERING", flag, &
                     "If true, neutral diffusion linearly decays to zero within a transition zone defined using boundary layer "//&
                     "depths.    Only applicable when NDIFF_INTERIOR_ONLY=True", default=.false.)
      CS%nd%unsupported(3) = merge(1, 0, flag)      ! CS%tapering
    endif
    CS%nd%unsupported(4) = merge(1, 0, CS%KhTr_use_ebt_struct)      ! CS%KhTh_use_ebt_struct: the same parameter (:199)
    call get_param(param_file, "MOM_neutral_diffusion", "NDIFF_USE_UNMASKED_TRANSPORT_BUG", flag, default=.false.)
    call refuse(flag, "NDIFF_USE_UNMASKED_TRANSPORT_BUG")
    call get_param(param_file, "MOM_neutral_diffusion", "NDIFF_ANSWER_DATE", CS%nd%ndiff_answer_date, &
                   "The vintage of the order of arithmetic to use for the neutral diffusion.", default=20240101)
    if (CS%nd%unsupported(1) /= 0) call ndiff_discontinuous_init()
    call mom6hip_read_eos(param_file, CS%eos, "neutral_diffusion_init")
    CS%nd%initialized = 1
  endif
  if (CS%use_neutral_diffusion .and. CS%Diffuse_ML_interior) call MOM_error(FATAL, "MOM_tracer_hor_diff: "// &
       "USE_NEUTRAL_DIFFUSION and DIFFUSE_ML_TO_INTERIOR are mutually exclusive!")
  call hor_bnd_diffusion_init()
  if (CS%use_hor_bnd_diffusion .and. CS%Diffuse_ML_interior) call MOM_error(FATAL, "MOM_tracer_hor_diff: "// &
       "USE_HORIZONTAL_BOUNDARY_DIFFUSION and DIFFUSE_ML_TO_INTERIOR are mutually exclusive!")
  call mom6hip_read_topology(param_file)
  call mom6hip_read_resident(param_file)
  id_clock_diffuse = cpu_clock_id('(Ocean diffuse tracer)', grain=CLOCK_MODULE)
contains
  !> hor_bnd_diffusion_init (src/tracer/MOM_hor_bnd_diffusion.F90:79-158): its parameters, names and defaults
  subroutine hor_bnd_diffusion_init()
    character(len=40) :: hbd_mdl = "MOM_hor_bnd_diffusion"
    character(len=80) :: string
    type(KPP_CS), pointer :: KPP_CSp => NULL()
    type(energetic_PBL_CS), pointer :: ePBL_CSp => NULL()
    logical :: debug
    call get_param(param_file, hbd_mdl, "USE_HORIZONTAL_BOUNDARY_DIFFUSION", CS%use_hor_bnd_diffusion, &
                   "If true, enables the horizonal boundary tracer's diffusion module.", default=.false.)
    if (.not.CS%use_hor_bnd_diffusion) return
    if (associated(diabatic_CSp)) then
      call extract_diabatic_member(diabatic_CSp, KPP_CSp=KPP_CSp)
      call extract_diabatic_member(diabatic_CSp, energetic_PBL_CSp=ePBL_CSp)
    endif
    if (.not.associated(ePBL_CSp) .and. .not.associated(KPP_CSp)) call MOM_error(FATAL, &
      "Horizontal boundary diffusion is true, but no valid boundary layer scheme was found")
    call get_param(param_file, hbd_mdl, "HBD_LINEAR_TRANSITION", flag, &
                   "If True, apply a linear transition at the base/top of the boundary. \n"//&
                   "The flux will be fully applied at k=k_min and zero at k=k_max.", default=.false.)
    CS%hbd%linear = merge(1, 0, flag)
    call get_param(param_file, hbd_mdl, "APPLY_LIMITER", flag, "If True, apply a flux limiter in the native grid.", default=.true.)
    CS%hbd%limiter = merge(1, 0, flag)
    call get_param(param_file, hbd_mdl, "APPLY_LIMITER_REMAP", flag, "If True, apply a flux limiter in the remapped grid.", &
                   default=.false.)
    CS%hbd%limiter_remap = merge(1, 0, flag)
    call get_param(param_file, hbd_mdl, "HBD_BOUNDARY_EXTRAP", flag, "Use boundary extrapolation in HBD code", default=.false.)
    CS%hbd%boundary_extrap = merge(1, 0, flag)
    call get_param(param_file, hbd_mdl, "HBD_REMAPPING_SCHEME", string, &
                   "This sets the reconstruction scheme used for vertical remapping for all variables.", default="PLM")
    select case (trim(string))
      case ("PCM") ; CS%hbd%remap_scheme = MOM6HIP_REMAP_PCM
      case ("PLM") ; CS%hbd%remap_scheme = MOM6HIP_REMAP_PLM
      case ("PPM_H4") ; CS%hbd%remap_scheme = MOM6HIP_REMAP_PPM_H4
      case ("PPM_IH4") ; CS%hbd%remap_scheme = MOM6HIP_REMAP_PPM_IH4
      case ("PPM_CW") ; CS%hbd%remap_scheme = MOM6HIP_REMAP_PPM_CW
      case default ; call refuse(.true., "HBD_REMAPPING_SCHEME = "//trim(string))
    end select
    call get_param(param_file, hbd_mdl, "DEBUG", debug, default=.false., do_not_log=.true.)
    call get_param(param_file, hbd_mdl, "HBD_DEBUG", flag, "If true, write out verbose debugging data in the HBD module.", &
                   default=debug)
    call refuse(flag, "HBD_DEBUG")
    CS%hbd%initialized = 1
  end subroutine hor_bnd_diffusion_init

  !> neutral_diffusion_init :219-277: the parameters read with NDIFF_CONTINUOUS = False, names, units and defaults
  subroutine ndiff_discontinuous_init()
    character(len=40) :: nd_mdl = "MOM_neutral_diffusion"
    character(len=80) :: string
    integer :: default_answer_date
    logical :: debug
    call refuse(CS%nd%unsupported(3) /= 0, "NDIFF_TAPERING with NDIFF_CONTINUOUS = False")
    call refuse(CS%KhTr_use_ebt_struct, "KHTR_USE_EBT_STRUCT with NDIFF_CONTINUOUS = False")
    call get_param(param_file, nd_mdl, "DEFAULT_ANSWER_DATE", default_answer_date, &
                   "This sets the default value for the various _ANSWER_DATE parameters.", default=99991231)
    call get_param(param_file, nd_mdl, "NDIFF_BOUNDARY_EXTRAP", flag, &
                   "Extrapolate at the top and bottommost cells, otherwise assume boundaries are piecewise constant", default=.false.)
    call refuse(flag, "NDIFF_BOUNDARY_EXTRAP = True")
    call get_param(param_file, nd_mdl, "NDIFF_REMAPPING_SCHEME", string, &
                   "This sets the reconstruction scheme used for vertical remapping for all variables.", default="PLM")
    select case (trim(string))
      case ("PLM") ; CS%ndd%remap_scheme = MOM6HIP_REMAP_PLM
      case ("PPM_H4") ; CS%ndd%remap_scheme = MOM6HIP_REMAP_PPM_H4
      case ("PPM_IH4") ; CS%ndd%remap_scheme = MOM6HIP_REMAP_PPM_IH4
      case default ; call refuse(.true., "NDIFF_REMAPPING_SCHEME = "//trim(string))
    end select
    call get_param(param_file, nd_mdl, "REMAPPING_ANSWER_DATE", CS%ndd%remap_answer_date, &
                   "The vintage of the expressions and order of arithmetic to use for remapping.", default=default_answer_date, &
                   do_not_log=.not.GV%Boussinesq)
    if (.not.GV%Boussinesq) CS%ndd%remap_answer_date = max(CS%ndd%remap_answer_date, 20230701)
    call refuse(CS%ndd%remap_answer_date < 20190101, "REMAPPING_ANSWER_DATE < 20190101 with NDIFF_CONTINUOUS = False")
    call get_param(param_file, nd_mdl, "NEUTRAL_POS_METHOD", CS%ndd%neutral_pos_method, &
                   "Method used to find the neutral position                 \n"// &
                   "1. Delta_rho varies linearly, find 0 crossing            \n"// &
                   "2. Alpha and beta vary linearly from top to bottom,      \n"// &
                   "   Newton's method for neutral position                  \n"// &
                   "3. Full nonlinear equation of state, use regula falsi    \n"// &
                   "   for neutral position", default=3)
    if (CS%ndd%neutral_pos_method > 4 .or. CS%ndd%neutral_pos_method < 0) call MOM_error(FATAL, "Invalid option for NEUTRAL_POS_METHOD")
    call refuse(CS%ndd%neutral_pos_method == 0 .or. CS%ndd%neutral_pos_method == 4, "NEUTRAL_POS_METHOD = 0 or 4")
    call get_param(param_file, nd_mdl, "DELTA_RHO_FORM", string, &
                   "Determine how the difference in density is calculated    \n"// &
                   "  full       : Difference of in-situ densities           \n"// &
                   "  no_pressure: Calculated from dRdT, dRdS, but no        \n"// &
                   "               pressure dependence", default="mid_pressure")
    select case (trim(string))
      case ("full") ; CS%ndd%delta_rho_form = MOM6HIP_DELTA_RHO_FULL
      case ("mid_pressure") ; CS%ndd%delta_rho_form = MOM6HIP_DELTA_RHO_MID_PRESSURE
      case ("local_pressure") ; CS%ndd%delta_rho_form = MOM6HIP_DELTA_RHO_LOCAL_PRESSURE
      case default ; call MOM_error(FATAL, "delta_rho_form is not recognized")
    end select
    call refuse(CS%ndd%neutral_pos_method == 2 .and. CS%ndd%delta_rho_form == MOM6HIP_DELTA_RHO_FULL, &
                "NEUTRAL_POS_METHOD = 2 with DELTA_RHO_FORM = full (the reference reads density derivatives this form never sets)")
    if (CS%ndd%neutral_pos_method > 1) then
      call get_param(param_file, nd_mdl, "NDIFF_DRHO_TOL", CS%ndd%drho_tol, &
                     "Sets the convergence criterion for finding the neutral position within a layer in kg m-3.", &
                     units="kg m-3", default=1.e-10, scale=US%kg_m3_to_R)
      call get_param(param_file, nd_mdl, "NDIFF_X_TOL", CS%ndd%x_tol, &
                     "Sets the convergence criterion for a change in nondimensional position within a layer.", &
                     units="nondim", default=0.)
      call get_param(param_file, nd_mdl, "NDIFF_MAX_ITER", CS%ndd%max_iter, &
                     "The maximum number of iterations to be done before exiting the iterative loop to find the neutral surface", &
                     default=10)
    endif
    call get_param(param_file, nd_mdl, "DEBUG", debug, default=.false., do_not_log=.true.)
    call get_param(param_file, nd_mdl, "NDIFF_DEBUG", debug, &
                   "Turns on verbose output for discontinuous neutral diffusion routines.", default=debug)      ! (only prints: ignored)
    call get_param(param_file, nd_mdl, "HARD_FAIL_HEFF", flag, "Bring down the model if a problem with heff is detected", default=.true.)
    CS%ndd%hard_fail_heff = merge(1, 0, flag)
    CS%ndd%initialized = 1
  end subroutine ndiff_discontinuous_init

  subroutine refuse(on, name)
    logical,          intent(in) :: on
    character(len=*), intent(in) :: name
    if (on) call MOM_error(FATAL, "tracer_hor_diff_init (HIP): "//name//" is not provided by the GPU path.")
  end subroutine refuse
end subroutine tracer_hor_diff_init

!> Same interface as the reference tracer_hor_diff_end (:1772)
subroutine tracer_hor_diff_end(CS)
  type(tracer_hor_diff_CS), pointer :: CS
  if (associated(CS)) deallocate(CS)
end subroutine tracer_hor_diff_end

end module MOM_tracer_hor_diff
