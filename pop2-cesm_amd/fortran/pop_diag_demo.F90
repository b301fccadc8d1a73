!|||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||
! Use of module diagnostics from Fortran: steps the small multi-block set-up 'tiny', arms the last
! step and prints diag_ke, avg_tracer(1:2), cfl_advt with its address and check_KE(100.) for the
! test suite to compare with the Python-driven run.
!   pop_diag_demo [nsteps]
!|||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||
 program pop_diag_demo

   use kinds_mod
   use pop_amd_c
   use blocks
   use step_mod, only: step
   use diagnostics
   implicit none

   type (pop_config) :: cfg
   integer (POP_i4) :: errorCode, nsteps, n, cfladd(3)
   real (POP_r8) :: cfl
   character (char_len) :: arg, msg

   nsteps = 4
   if (command_argument_count() >= 1) then
      call get_command_argument(1, arg)
      read(arg, *) nsteps
   endif
   cfg = tiny_config()
   errorCode = pop_create(cfg, 0, 1, 0, pop_ctx)
   if (errorCode /= POP_Success) call fail('pop_create')
   call init_blocks_from_ctx
   if (.not. check_KE(100.0_r8)) call fail('check_KE before an armed step must not pass')
   do n = 1, nsteps
      if (n == nsteps) then
         call diag_arm(.true., .true., errorCode)
         if (errorCode /= POP_Success) call fail('diag_arm')
      endif
      call step(errorCode)
      if (errorCode /= POP_Success) call fail('step')
   end do
   cfl = cfl_advt(cfladd)
   write(*,'(a,es24.16,a,es24.16,a,es24.16,a,es24.16,a,3i6,a,l2)') 'diag_ke ', diag_ke(), ' avg_tracer1 ', avg_tracer(1), &
      ' avg_tracer2 ', avg_tracer(2), ' cfl_advt ', cfl, ' cfladd_advt ', cfladd, ' check_KE ', check_KE(100.0_r8)
   if (check_KE(100.0_r8)) write(*,*) 'the run would stop here'
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

 end program pop_diag_demo
