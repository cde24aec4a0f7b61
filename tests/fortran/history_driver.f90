! TEST INFRASTRUCTURE: dev_driver.f90's device-resident time loop with the four accumulators of the reference's WRF_HYDRO build
! (ACCPRCP, ACCECAN, ACCETRAN, ACCEDIR: drv:736-739) kept on the device through the generated interfaces of the device-side history
! (noahmp_hip_history_step): per step forcing preparation, the column step and one history sample, all only enqueued; one
! synchronisation at the end, then the four planes and the state come back.
function history_driver_run(a, lon2d, rain_rate, nsteps, iday0, zlvl, acc4) bind(C, name='history_driver_run') result(rc)
  use iso_c_binding
  use noahmp_hip_abi
  use noahmp_hip_device
  implicit none
  type(noahmp_step_args), intent(in) :: a            ! host arrays
  type(c_ptr), value :: lon2d, rain_rate             ! host planes (ims:ime, jms:jme)
  integer(c_int), value :: nsteps, iday0
  real(c_float), value :: zlvl
  type(c_ptr), value :: acc4                         ! host: four planes back to back (accprcp, accecan, accetran, accedir), in: start values
  integer(c_int) :: rc
  type(noahmp_step_args) :: d
  type(noahmp_status) :: st
  type(noahmp_history_entry) :: e(4)
  type(c_ptr) :: dlon, drain, dacc
  real(c_float), pointer :: hacc(:)
  integer(c_size_t) :: nb, ncol
  integer(c_int) :: n, f, flags, bad_step
  real(c_float) :: jul

  call noahmp_hip_block_to_device(a, d, rc)
  if (rc /= 0) return
  ncol = int(a%ime - a%ims + 1, c_size_t) * int(a%jme - a%jms + 1, c_size_t)
  nb = 4_c_size_t * ncol
  dlon = noahmp_hip_malloc(nb); drain = noahmp_hip_malloc(nb); dacc = noahmp_hip_malloc(4_c_size_t * nb)
  rc = noahmp_hip_memcpy(dlon, lon2d, nb, 0_c_int)
  if (rc == 0) rc = noahmp_hip_memcpy(drain, rain_rate, nb, 0_c_int)
  if (rc == 0) rc = noahmp_hip_memcpy(dacc, acc4, 4_c_size_t * nb, 0_c_int)
  call c_f_pointer(acc4, hacc, [4_c_size_t * ncol])
  ! ACCPRCP: the forcing plane RAINBL is fl(PRCP * DT) already (hdrv:343): a plain sum; the others: ACC + X * DT
  e(1)%src = d%rainbl;  e(1)%op = NOAHMP_HIST_SUM
  e(2)%src = d%ecanxy;  e(2)%op = NOAHMP_HIST_SUM_DT
  e(3)%src = d%etranxy; e(3)%op = NOAHMP_HIST_SUM_DT
  e(4)%src = d%edirxy;  e(4)%op = NOAHMP_HIST_SUM_DT
  do f = 1, 4
     e(f)%acc = transfer(transfer(dacc, 0_c_intptr_t) + int(f - 1, c_intptr_t) * int(nb, c_intptr_t), c_null_ptr)
     e(f)%nlev = 1
     e(f)%scale = a%dt
  end do
  do n = 0, nsteps - 1
     if (rc /= 0) exit
     flags = 0
     if (n == 0) flags = NOAHMP_PREP_FIRST_STEP
     rc = noahmp_hip_forcing_prep(d, dlon, drain, iday0 + n / 24, mod(n, 24), 0_c_int, 0_c_int, zlvl, flags, jul, &
                                  1_c_int, c_null_ptr, c_null_ptr)
     if (rc /= 0) exit
     d%itimestep = n + 1
     d%julian = jul
     rc = noahmp_hip_step_async(d, c_null_ptr)
     if (rc /= 0) exit
     rc = noahmp_hip_history_step(4_c_int, e, c_null_ptr, d, c_null_ptr, c_null_ptr)
  end do
  if (rc == 0) rc = noahmp_hip_sync(st, bad_step)
  if (rc == 0) rc = noahmp_hip_memcpy(acc4, dacc, 4_c_size_t * nb, 1_c_int)
  if (rc == 0) call noahmp_hip_block_from_device(d, a, rc)
  call noahmp_hip_block_free(d)
  call noahmp_hip_free(dlon); call noahmp_hip_free(drain); call noahmp_hip_free(dacc)
end function history_driver_run
