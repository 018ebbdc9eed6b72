!! Voxel-grid clusters of a batch of point clouds from FORTRAN through the C ABI: what a caller that holds Fortran arrays does to
!! coarsen large clouds -- query the number of clusters, allocate, fill -- and to carry a gradient of the centroids back to the
!! points.
!!
!!   grid_clusters_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_clouds, n, dim, has_origin; real32 size, origin(3) (ignored unless has_origin = 1);
!!                       int32 offsets(n_clouds + 1); real32 points(dim, n)
!! result file (stream): int64 m; int32 cluster(n), adj_ia(m + 1), adj_ja(2, n); real32 weights(n), centroid(dim, m);
!!                       int32 nearest(m), cell(dim, m), cluster_offsets(n_clouds + 1); real32 origin_out(dim, n_clouds),
!!                       dpoints(dim, n) (the reverse step of dcentroid(k, c) = k + c); int64 stats(4)
!! tests/test_gpu_grid_clusters.py compares the arrays with the yardstick's.
program grid_clusters_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit, c, k
  integer(c_int32_t) :: n_clouds, n, dim, has_origin
  integer(c_int64_t) :: m, m_again
  real(c_float) :: cell_size
  real(c_float), target :: origin(3)
  integer(c_int32_t), allocatable :: offsets(:)
  integer(c_int32_t), allocatable, target :: cluster(:), adj_ia(:), adj_ja(:,:), nearest(:), cell(:,:), cluster_offsets(:)
  real(c_float), allocatable :: points(:,:), dcentroid(:,:), dpoints(:,:)
  real(c_float), allocatable, target :: weights(:), centroid(:,:), origin_out(:,:)
  integer(c_int64_t) :: stats(4)
  type(c_ptr) :: origin_ptr

  if(command_argument_count() .lt. 2) stop "usage: grid_clusters_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_clouds, n, dim, has_origin
  read(unit) cell_size, origin
  allocate(offsets(n_clouds + 1), points(dim, n))
  read(unit) offsets
  read(unit) points
  close(unit)
  origin_ptr = c_null_ptr
  if(has_origin .eq. 1) origin_ptr = c_loc(origin)

  call must(athena_mp_init(0_c_int), "init")
  allocate(cluster_offsets(n_clouds + 1), origin_out(dim, n_clouds))
  ! the size query: adj_ja = c_null_ptr
  call must(athena_mp_grid_clusters_host(n_clouds, n, offsets, dim, points, cell_size, origin_ptr, 0_c_int64_t, c_null_ptr, c_null_ptr, &
       c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_loc(cluster_offsets), c_loc(origin_out), m), "grid_clusters_host (query)")
  allocate(cluster(n), adj_ia(m + 1), adj_ja(2, n), weights(n), centroid(dim, m), nearest(m), cell(dim, m))
  call must(athena_mp_grid_clusters_host(n_clouds, n, offsets, dim, points, cell_size, origin_ptr, m, c_loc(cluster), c_loc(adj_ia), &
       c_loc(adj_ja), c_loc(weights), c_loc(centroid), c_loc(nearest), c_loc(cell), c_loc(cluster_offsets), c_loc(origin_out), &
       m_again), "grid_clusters_host")
  if(m_again .ne. m) stop "the fill found another number of clusters than the query"
  call must(athena_mp_grid_clusters_stats(stats), "grid_clusters_stats")
  allocate(dcentroid(dim, m), dpoints(dim, n))
  do c = 1, int(m)
     do k = 1, dim
        dcentroid(k, c) = real(k + c, c_float)
     end do
  end do
  call must(athena_mp_grid_clusters_grad_host(n, dim, int(m, c_int32_t), cluster, adj_ia, dcentroid, dpoints), "grid_clusters_grad_host")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) m, cluster, adj_ia, adj_ja, weights, centroid, nearest, cell, cluster_offsets, origin_out, dpoints, stats
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A)') "grid clusters: ", n_clouds, " clouds, ", n, " points, ", m, " clusters"
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
end program grid_clusters_run
