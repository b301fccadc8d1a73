!|||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||
! Use of compute_tracer_transports of module diags_on_lat_aux_grid from Fortran: steps the small multi-block set-up
! 'tiny' with N_HEAT and N_SALT in tavg stream 1 ('southern' auxiliary grid, one region, no MOC), and prints the
! sizes, tavg_sum, the number of masked entries and three numbers of each of TAVG_N_HEAT_TRANS_G and
! TAVG_N_SALT_TRANS_G for the test suite to compare with the Python-driven run.
!   pop_transport_demo [nsteps]
!|||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||
 program pop_transport_demo

   use kinds_mod
   use pop_amd_c
   use blocks
   use step_mod, only: step
   use tavg, only: tavg_sum
   use diags_on_lat_aux_grid
   implicit none

   type (pop_config) :: cfg
   integer (POP_i4) :: errorCode, nsteps, n, nmid
   character (char_len) :: arg, msg

   nsteps = 3
   if (command_argument_count() >= 1) then
      call get_command_argument(1, arg)
      read(arg, *) nsteps
   endif
   cfg = tiny_config()
   errorCode = pop_create(cfg, 0, 1, 0, pop_ctx)
   if (errorCode /= POP_Success) call fail('pop_create')
   call init_blocks_from_ctx
   call init_transports_nml
   transports%n_transport_reg = 1
   moc_requested = .false.
   n_heat_trans_requested = .true.; n_salt_trans_requested = .true.
   call init_lat_aux_grid(errorCode)
   if (errorCode /= POP_Success) call fail('init_lat_aux_grid')
   call init_moc_ts_transport_arrays(errorCode)
   if (errorCode /= POP_Success) call fail('init_moc_ts_transport_arrays')
   do n = 1, nsteps
      call step(errorCode)
      if (errorCode /= POP_Success) call fail('step')
   end do
   call compute_tracer_transports(1, errorCode)
   if (errorCode /= POP_Success) call fail('compute_tracer_transports(1)')
   call compute_tracer_transports(2, errorCode)
   if (errorCode /= POP_Success) call fail('compute_tracer_transports(2)')
   nmid = n_lat_aux_grid/2
   write(*,'(a,i6,a,i3,a,i3,a,es23.15,a,i6)') 'n_lat_aux_grid ', n_lat_aux_grid, ' n_transport_comp ', n_transport_comp, &
      ' n_transport_reg ', n_transport_reg, ' tavg_sum ', tavg_sum(1), ' masked ', count(TAVG_N_HEAT_TRANS_G == undefined_nf)
   write(*,'(a,es16.8,a,es16.8,a,es16.8)') 'heat_total_mid ', TAVG_N_HEAT_TRANS_G(nmid,1,1), ' heat_adv_mid ', &
      TAVG_N_HEAT_TRANS_G(nmid,2,1), ' heat_dif_mid ', TAVG_N_HEAT_TRANS_G(nmid,3,1)
   write(*,'(a,es16.8,a,es16.8,a,es16.8)') 'salt_total_mid ', TAVG_N_SALT_TRANS_G(nmid,1,1), ' salt_adv_mid ', &
      TAVG_N_SALT_TRANS_G(nmid,2,1), ' salt_dif_mid ', TAVG_N_SALT_TRANS_G(nmid,3,1)
   errorCode = pop_destroy(pop_ctx)

 contains

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

 end program pop_transport_demo
