!! The k-nearest-neighbour graphs of a batch of point clouds as ONE block-diagonal graph from FORTRAN through the C ABI: what a
!! caller that holds Fortran arrays does in front of graph_nop_layer_type's set_graph for clouds of uneven density -- query,
!! allocate, fill.
!!
!!   knn_graph_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_clouds, n, dim, k, mode, add_self_loops; real32 radius (+infinity: no cap);
!!                       int32 offsets(n_clouds + 1); real32 points(dim, n)
!! result file (stream): int32 n_clouds, n, dim, nnz, pairs; int32 adj_ia(n + 1), adj_ja(2, nnz); real32 coords(dim, pairs);
!!                       int64 edge_offsets(n_clouds + 1); int64 stats(4)
!! tests/test_gpu_knn_graph.py compares the arrays with the yardstick's.
program knn_graph_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n_clouds, n, dim, k, mode, loops
  real(c_float) :: radius
  integer(c_int32_t), allocatable :: offsets(:)
  real(c_float), allocatable :: points(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:)
  real(c_float), allocatable, target :: coords(:,:)
  integer(c_int64_t), allocatable, target :: edge_offsets(:)
  integer(c_int64_t) :: nnz, pairs, stats(4)

  if(command_argument_count() .lt. 2) stop "usage: knn_graph_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_clouds, n, dim, k, mode, loops
  read(unit) radius
  allocate(offsets(n_clouds + 1), points(dim, n), edge_offsets(n_clouds + 1))
  read(unit) offsets
  read(unit) points
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_knn_graph_batched_host(n_clouds, n, offsets, dim, points, k, radius, mode, loops, c_null_ptr, c_null_ptr, &
       0_c_int64_t, nnz, c_null_ptr, 0_c_int64_t, pairs, c_null_ptr), "knn_graph_batched_host (size query)")
  allocate(adj_ia(n + 1), adj_ja(2, nnz), coords(dim, pairs))
  call must(athena_mp_knn_graph_batched_host(n_clouds, n, offsets, dim, points, k, radius, mode, loops, c_loc(adj_ia), &
       c_loc(adj_ja), nnz, nnz, c_loc(coords), pairs, pairs, c_loc(edge_offsets)), "knn_graph_batched_host")
  call must(athena_mp_knn_stats(stats), "knn_stats")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) n_clouds, n, dim, int(nnz, c_int32_t), int(pairs, c_int32_t)
  write(unit) adj_ia, adj_ja, coords, edge_offsets, stats
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A,I0,A)') "k-nearest-neighbour graphs: ", n_clouds, " clouds, ", n, " points, k = ", k, ", ", &
       pairs, " pairs, ", nnz, " entries"
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
end program knn_graph_run
