!! Farthest-point samples of a batch of point clouds from FORTRAN through the C ABI: what a caller that holds Fortran arrays does
!! to get the second point set of athena_mp_radius_graph_bipartite_host / athena_mp_knn_graph_bipartite_host, and the radius
!! that covers every point.
!!
!!   fps_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_clouds, n, dim, n_samples, has_start; int32 offsets(n_clouds + 1), sample_offsets(n_clouds + 1),
!!                       start(n_clouds) (1-based global, 0: the cloud's first point; ignored unless has_start = 1);
!!                       real32 points(dim, n)
!! result file (stream): int32 sample(n_samples); real32 sample_points(dim, n_samples), sample_sqdist(n_samples),
!!                       cover_sqdist(n_clouds); int64 stats(4)
!! tests/test_gpu_fps.py compares the arrays with the yardstick's.
program fps_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n_clouds, n, dim, n_samples, has_start
  integer(c_int32_t), allocatable :: offsets(:), sample_offsets(:)
  integer(c_int32_t), allocatable, target :: start(:), sample(:)
  real(c_float), allocatable :: points(:,:)
  real(c_float), allocatable, target :: sample_points(:,:), sample_sqdist(:), cover_sqdist(:)
  integer(c_int64_t) :: stats(4)
  type(c_ptr) :: start_ptr

  if(command_argument_count() .lt. 2) stop "usage: fps_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_clouds, n, dim, n_samples, has_start
  allocate(offsets(n_clouds + 1), sample_offsets(n_clouds + 1), start(n_clouds), points(dim, n))
  read(unit) offsets, sample_offsets, start
  read(unit) points
  close(unit)
  start_ptr = c_null_ptr
  if(has_start .eq. 1) start_ptr = c_loc(start)

  call must(athena_mp_init(0_c_int), "init")
  allocate(sample(n_samples), sample_points(dim, n_samples), sample_sqdist(n_samples), cover_sqdist(n_clouds))
  call must(athena_mp_farthest_points_host(n_clouds, n, offsets, dim, points, n_samples, sample_offsets, start_ptr, &
       c_loc(sample), c_loc(sample_points), c_loc(sample_sqdist), c_loc(cover_sqdist)), "farthest_points_host")
  call must(athena_mp_fps_stats(stats), "fps_stats")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) sample, sample_points, sample_sqdist, cover_sqdist, stats
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A)') "farthest-point samples: ", n_clouds, " clouds, ", n, " points, ", n_samples, " samples"
  call must(athena_mp_finalize(), "finalize")

contains

  subroutine must(rc, what)
    integer(c_int), intent(in) :: rc
    character(*), intent(in) :: what
    if(rc .ne. 0)then
       write(0,*) what//" failed: "//athena_mp_error_message()
       stop 1
    end if
  end subroutine must
end program fps_run
