!|||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||
! Use of the modules forcing_coupled, forcing, ice and ms_balance from Fortran, as a coupler cap would: the small multi-block set-up
! 'tiny' in CESM's form -- the virtual salt flux (lfw_as_salt_flx) with the marginal-sea balance -- on a REGION_MASK with two marginal
! seas built from KMT by index arithmetic (the mask of tests/forcing_common.py ms_setup), x2o fields that are exact rational
! functions of the cell's address handed over through rotate_wind_stress / coupler_field, pop_set_coupled_forcing, then nsteps
! steps.  Prints the seas (number, points, first point, area, warnings, transport), checksums of STF, SMF, SMFT and SHF_QSW and the
! interval's step count for the test suite to compare with the Python-driven run.
!   pop_forcing_demo [nsteps]
!|||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||
 program pop_forcing_demo

   use kinds_mod
   use pop_amd_c
   use blocks
   use step_mod, only: step
   use ice, only: init_ice, ice_freq_opt, licecesm2, lfw_as_salt_flx
   use ms_balance
   use forcing_coupled
   use forcing, only: set_surface_forcing
   implicit none

   type (pop_config) :: cfg
   integer (POP_i4) :: errorCode, nsteps, n, f, info(4), nseas, number, warnings
   character (char_len) :: arg, msg
   character (8), parameter :: names(15) = [character(8) :: 'snow', 'rain', 'evap', 'meltw', 'rofl', 'rofi', 'salt', 'swnet', 'sen', &
                                            'lwup', 'lwdn', 'melth', 'ifrac', 'pslv', 'duu10n']
   real (r8), parameter :: amp(17) = [0.2_r8, 0.2_r8, 2.0e-5_r8, 8.0e-5_r8, 6.0e-5_r8, 3.0e-5_r8, 2.0e-5_r8, 1.0e-5_r8, 1.0e-6_r8, &
                                      250.0_r8, 40.0_r8, 400.0_r8, 350.0_r8, 30.0_r8, 0.5_r8, 1.0e5_r8, 60.0_r8]
   real (r8), dimension(:,:,:,:), allocatable, target :: X
   real (r8), dimension(:,:,:), allocatable :: A
   integer (POP_i4), dimension(:,:), allocatable :: REGION_MASK_G
   integer (POP_i4) :: reg_numbers(4)
   character (8) :: reg_names(4)
   real (r8) :: reg_lat(4), reg_lon(4), reg_area(4), area, transport(2)
   integer (POP_i4), dimension(:), allocatable :: ipts, jpts
   real (r8), dimension(:), allocatable :: fracs

   nsteps = 2
   if (command_argument_count() >= 1) then
      call get_command_argument(1, arg)
      read(arg, *) nsteps
   endif
   cfg = tiny_config()
   errorCode = pop_create(cfg, 0, 1, 0, pop_ctx)
   if (errorCode /= POP_Success) call fail('pop_create')
   call init_blocks_from_ctx
   ice_freq_opt = 'coupled'; licecesm2 = .true.; lfw_as_salt_flx = .true.
   call init_ice(errorCode)
   if (errorCode /= POP_Success) call fail('init_ice')
   allocate(X(nx_block, ny_block, nblocks_clinic, 17), A(nx_block, ny_block, nblocks_clinic))
   call region_table
   call init_ms_balance(reg_numbers, reg_names, reg_lat, reg_lon, reg_area, REGION_MASK_G, errorCode)
   if (errorCode /= POP_Success) call fail('init_ms_balance')
   lms_balance = .true.
   call pop_init_coupled(errorCode)
   if (errorCode /= POP_Success) call fail('pop_init_coupled')
   do f = 1, 17
      call fill(X(:,:,:,f), f)
   end do
   call rotate_wind_stress(X(:,:,:,1), X(:,:,:,2))
   do f = 3, 17
      call coupler_field(trim(names(f-2)), X(:,:,:,f), errorCode)
      if (errorCode /= POP_Success) call fail('coupler_field')
   end do
   call update_ghost_cells_coupler_fluxes(errorCode)
   call pop_set_coupled_forcing(errorCode)
   if (errorCode /= POP_Success) call fail('pop_set_coupled_forcing')
   call ms_balancing(transport, errorCode)
   if (errorCode /= POP_Success) call fail('ms_balancing')
   do n = 1, 2
      call ms_balance_sea(n, number, area, warnings, ipts, jpts, fracs, errorCode)
      if (errorCode /= POP_Success) call fail('ms_balance_sea')
      write(*,'(a,i4,a,i5,a,i4,i4,a,es24.16,a,es24.16,a,i3,a,es24.16)') 'sea ', number, ' npts ', size(ipts), ' first ', ipts(1), jpts(1), &
         ' lastfrac ', fracs(size(fracs)), ' area ', area, ' warnings ', warnings, ' transport ', transport(n)
   end do
   call checksum('STF', 1, 'stf2_import')
   do n = 1, nsteps
      call step(errorCode)
      if (errorCode /= POP_Success) call fail('step')
   end do
   call set_surface_forcing(errorCode)
   if (errorCode /= POP_Success) call fail('set_surface_forcing')
   errorCode = pop_coupled_info(pop_ctx, info, nseas)
   write(*,'(a,i4,a,i4,a,i4)') 'nsteps_per_interval ', info(3), ' nsteps_this_interval ', info(4), ' n_marginal_seas ', nseas
   call checksum('STF', 0, 'stf1'); call checksum('STF', 1, 'stf2'); call checksum('FW', 0, 'fw')
   call checksum('SMF', 0, 'smf1'); call checksum('SMF', 1, 'smf2')
   call checksum('SMFT', 0, 'smft1'); call checksum('SMFT', 1, 'smft2'); call checksum('SHF_QSW', 0, 'shf_qsw')
   errorCode = pop_destroy(pop_ctx)

 contains

   ! tests/forcing_common.py ms_setup: open ocean 1, region 2 from global i = 14 on, land 0, marginal sea -3 on i 11 .. 14, j 19 .. 22
   ! (the corner of four blocks) and -5 on i 5 .. 7, j 26 .. 28; each sea's search centre is the T point two rows north of it and one
   ! column east, the area asked for 7.5 cells of that size
   subroutine region_table
      integer (POP_i4), dimension(:,:,:), allocatable :: KMT
      integer (POP_i4), dimension(:,:), allocatable :: KMT_G
      real (r8), dimension(:,:), allocatable :: TLAT_G, AREA_G
      real (r8), dimension(:,:,:), allocatable :: TLAT, DXT, DYT
      integer (c_int), dimension(:), allocatable :: ids
      type (block) :: this_block
      integer (POP_i4) :: lb, i, j, ig, jg, s, ic, jc
      integer (POP_i4), parameter :: si(2,2) = reshape([11, 14, 5, 7], [2,2]), sj(2,2) = reshape([19, 22, 26, 28], [2,2]), snum(2) = [-3, -5]
      real (r8) :: radian, dlon
      allocate(KMT(nx_block, ny_block, nblocks_clinic), TLAT(nx_block, ny_block, nblocks_clinic))
      allocate(DXT(nx_block, ny_block, nblocks_clinic), DYT(nx_block, ny_block, nblocks_clinic), ids(nblocks_clinic))
      allocate(KMT_G(cfg%nx_global, cfg%ny_global), TLAT_G(cfg%nx_global, cfg%ny_global), AREA_G(cfg%nx_global, cfg%ny_global))
      allocate(REGION_MASK_G(cfg%nx_global, cfg%ny_global))
      errorCode = pop_get_ifield(pop_ctx, cstr('KMT'), KMT, int(size(KMT), c_long_long))
      if (errorCode /= POP_Success) call fail('pop_get_ifield KMT')
      errorCode = pop_get_field(pop_ctx, cstr('TLAT'), 1, 0, TLAT, int(size(TLAT), c_long_long))
      if (errorCode == POP_Success) errorCode = pop_get_field(pop_ctx, cstr('DXT'), 1, 0, DXT, int(size(DXT), c_long_long))
      if (errorCode == POP_Success) errorCode = pop_get_field(pop_ctx, cstr('DYT'), 1, 0, DYT, int(size(DYT), c_long_long))
      if (errorCode /= POP_Success) call fail('pop_get_field TLAT / DXT / DYT')
      errorCode = pop_local_block_ids(pop_ctx, ids)
      KMT_G = 0; TLAT_G = 0.0_r8; AREA_G = 0.0_r8
      do lb = 1, nblocks_clinic                      ! gather_global: the physical cells of every block
         this_block = get_block(ids(lb), lb)
         do j = this_block%jb, this_block%je
            do i = this_block%ib, this_block%ie
               ig = this_block%i_glob(i); jg = this_block%j_glob(j)
               if (ig < 1 .or. jg < 1) cycle
               KMT_G(ig,jg) = KMT(i,j,lb); TLAT_G(ig,jg) = TLAT(i,j,lb); AREA_G(ig,jg) = DXT(i,j,lb)*DYT(i,j,lb)
            end do
         end do
         deallocate(this_block%i_glob, this_block%j_glob)
      end do
      REGION_MASK_G = merge(1, 0, KMT_G > 0)
      where (KMT_G(14:,:) > 0) REGION_MASK_G(14:,:) = 2
      radian = 180.0_r8/(4.0_r8*atan(1.0_r8)); dlon = 360.0_r8/real(cfg%nx_global, r8)
      reg_numbers(1:2) = [1, 2]; reg_names(1:2) = [character(8) :: 'open', 'east']
      reg_lat(1:2) = 0.0_r8; reg_lon(1:2) = 0.0_r8; reg_area(1:2) = 0.0_r8
      do s = 1, 2
         where (KMT_G(si(1,s):si(2,s), sj(1,s):sj(2,s)) > 0) REGION_MASK_G(si(1,s):si(2,s), sj(1,s):sj(2,s)) = snum(s)
         ic = si(2,s) + 1; jc = sj(2,s) + 2
         reg_numbers(2+s) = snum(s)
         write(reg_names(2+s), '(a,i1)') 'sea', -snum(s)
         reg_lat(2+s) = TLAT_G(ic,jc)*radian
         reg_lon(2+s) = (real(ic - 1, r8) + 0.5_r8)*dlon
         reg_area(2+s) = 7.5_r8*AREA_G(ic,jc)
      end do
   end subroutine


   ! amp(f) * (mod(7 i + 13 j + 5 b + 3 f, 17) - 8) / 8: the same bits from any language
   subroutine fill(F3, f)
      real (r8), dimension(:,:,:), intent(out) :: F3
      integer (POP_i4), intent(in) :: f
      integer (POP_i4) :: i, j, b
      do b = 1, size(F3, 3)
         do j = 1, size(F3, 2)
            do i = 1, size(F3, 1)
               F3(i,j,b) = amp(f) * real(mod(7*i + 13*j + 5*b + 3*f, 17) - 8, r8) / 8.0_r8
            end do
         end do
      end do
   end subroutine

   subroutine checksum(name, n, label)
      character (*), intent(in) :: name, label
      integer (POP_i4), intent(in) :: n
      errorCode = pop_get_field(pop_ctx, cstr(name), 1, n, A, int(size(A), c_long_long))
      if (errorCode /= POP_Success) call fail('pop_get_field ' // name)
      write(*,'(a,a,es24.16,a,es24.16)') label, ' sum ', sum(A), ' sumabs ', sum(abs(A))
   end subroutine

   subroutine fail(what)
      character (*), intent(in) :: what
      call pop_amd_error_message(msg)
      write(*,*) what, ' failed: ', trim(msg)
      stop 1
   end subroutine

   ! tests/popcfg.py named_config('tiny')
   function tiny_config() result(c)
      type (pop_config) :: c
      c%nx_global = 48; c%ny_global = 40; c%km = 16; c%nt = 2
      c%block_size_x = 12; c%block_size_y = 10
      c%ew_boundary = 1; c%ns_boundary = 0
      c%hmix_momentum = 2; c%hmix_tracer = 2; c%lvariable_hmix = 0
      c%vmix_choice = 1; c%tadvect = 1; c%solver_choice = 1
      c%max_iterations = 1000; c%convergence_check_freq = 10
      c%tmix_opt = 2; c%time_mix_freq = 17; c%steps_per_day = 24
      c%lbouss_correct = 0; c%lpressure_avg = 1; c%impcor = 1; c%reset_to_freezing = 1
      c%lrich = 1; c%ldbl_diff = 0; c%lshort_wave = 0; c%lcheckekmo = 0; c%num_v_smooth_Ri = 1
      c%am = 3.0e9_c_double; c%ah = 1.0e7_c_double
      c%const_vvc = 0.25_c_double; c%const_vdc = 0.25_c_double
      c%convect_diff = 1000.0_c_double; c%convect_visc = 1000.0_c_double
      c%bottom_drag = 1.0e-3_c_double; c%aidif = 1.0_c_double
      c%rich_bckgrnd_vvc = 1.0_c_double; c%rich_bckgrnd_vdc = 0.1_c_double; c%rich_mix = 50.0_c_double
      c%bckgrnd_vdc1 = 0.1_c_double; c%bckgrnd_vdc2 = 0.0_c_double
      c%bckgrnd_vdc_dpth = 2500.0e2_c_double; c%bckgrnd_vdc_linv = 4.5e-5_c_double
      c%Prandtl = 10.0_c_double; c%kpp_rich_mix = 50.0_c_double
      c%convergence_criterion = 1.0e-12_c_double
      c%init_ts_perturbation = 1.0e-2_c_double
   end function tiny_config

 end program pop_forcing_demo
