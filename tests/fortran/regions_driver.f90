! TEST INFRASTRUCTURE: dev_driver.f90's device-resident time loop that keeps a per-step basin series of RUNSFXY on the device through the
! generated interfaces of the region series (noahmp_hip_region_plan / noahmp_hip_region_step): per step forcing preparation, the column
! step and one ring slot, all only enqueued; one synchronisation at the end, then the ring [nsteps][2][nregion] (entry 1: area-weighted
! sum of RUNSFXY, entry 2: the summed weights of the cells that took part -- their quotient is the basin mean) and the state come back.
function regions_driver_run(a, lon2d, rain_rate, nsteps, iday0, zlvl, region, weight, nregion, series) &
    bind(C, name='regions_driver_run') result(rc)
  use iso_c_binding
  use noahmp_hip_abi
  use noahmp_hip_device
  implicit none
  type(noahmp_step_args), intent(in) :: a            ! host arrays
  type(c_ptr), value :: lon2d, rain_rate             ! host planes (ims:ime, jms:jme)
  integer(c_int), value :: nsteps, iday0, nregion
  real(c_float), value :: zlvl
  type(c_ptr), value :: region, weight               ! host planes in tile order: int32 basin ids (negative: none), float32 cell areas
  type(c_ptr), value :: series                       ! host: float64 [nsteps][2][nregion]
  integer(c_int) :: rc
  type(noahmp_step_args) :: d
  type(noahmp_status) :: st
  type(noahmp_region_entry) :: e(2)
  type(c_ptr) :: dlon, drain, dregion, dweight, dplan, dseries, dscratch
  integer(c_size_t) :: nb, ncol, sb
  integer(c_int64_t) :: words, sbytes
  integer(c_int) :: n, flags, bad_step, ni, nj
  real(c_float) :: jul

  call noahmp_hip_block_to_device(a, d, rc)
  if (rc /= 0) return
  ni = a%ime - a%ims + 1; nj = a%jme - a%jms + 1
  ncol = int(ni, c_size_t) * int(nj, c_size_t)
  nb = 4_c_size_t * ncol
  sb = 8_c_size_t * int(nsteps, c_size_t) * 2_c_size_t * int(nregion, c_size_t)
  dplan = c_null_ptr; dscratch = c_null_ptr
  dlon = noahmp_hip_malloc(nb); drain = noahmp_hip_malloc(nb); dregion = noahmp_hip_malloc(nb); dweight = noahmp_hip_malloc(nb)
  dseries = noahmp_hip_malloc(sb)
  rc = noahmp_hip_memcpy(dlon, lon2d, nb, 0_c_int)
  if (rc == 0) rc = noahmp_hip_memcpy(drain, rain_rate, nb, 0_c_int)
  if (rc == 0) rc = noahmp_hip_memcpy(dregion, region, nb, 0_c_int)
  if (rc == 0) rc = noahmp_hip_memcpy(dweight, weight, nb, 0_c_int)
  ! the plan: once, on the device, tile order (no sort here: inv_perm = NULL)
  if (rc == 0) rc = noahmp_hip_region_plan_size(ni, nj, nregion, words)
  if (rc == 0) then
     dplan = noahmp_hip_malloc(4_c_size_t * int(words, c_size_t))
     rc = noahmp_hip_region_plan(dregion, dweight, ni, nj, nregion, c_null_ptr, dplan, words, c_null_ptr)
  end if
  if (rc == 0) rc = noahmp_hip_region_scratch_size(dplan, 2_c_int, sbytes)
  if (rc == 0) dscratch = noahmp_hip_malloc(int(sbytes, c_size_t))
  e(1)%src = d%runsfxy;  e(1)%nlev = 1; e(1)%lev = 0; e(1)%op = NOAHMP_REG_SUM
  e(2)%src = c_null_ptr; e(2)%nlev = 1; e(2)%lev = 0; e(2)%op = NOAHMP_REG_SUM      ! the constant 1: the summed weights
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
     rc = noahmp_hip_region_step(dplan, 2_c_int, e, d, dseries, nsteps, n, c_null_ptr, dscratch, c_null_ptr)
  end do
  if (rc == 0) rc = noahmp_hip_sync(st, bad_step)
  if (rc == 0) rc = noahmp_hip_memcpy(series, dseries, sb, 1_c_int)
  if (rc == 0) call noahmp_hip_block_from_device(d, a, rc)
  call noahmp_hip_block_free(d)
  call noahmp_hip_free(dlon); call noahmp_hip_free(drain); call noahmp_hip_free(dregion); call noahmp_hip_free(dweight)
  call noahmp_hip_free(dseries); call noahmp_hip_free(dplan); call noahmp_hip_free(dscratch)
end function regions_driver_run
