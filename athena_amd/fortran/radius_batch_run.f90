!! The radius graphs of a batch of point clouds as ONE block-diagonal graph from FORTRAN through the C ABI: what a caller that
!! holds Fortran arrays does in front of graph_nop_layer_type's set_graph for a dataset of clouds -- query, allocate, fill.
!!
!!   radius_batch_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_clouds, n, dim, add_self_loops; real32 radius; int32 offsets(n_clouds + 1); real32 points(dim, n)
!! result file (stream): int32 n_clouds, n, dim, nnz, pairs; int32 adj_ia(n + 1), adj_ja(2, nnz); real32 coords(dim, pairs);
!!                       int64 edge_offsets(n_clouds + 1)
!! tests/test_gpu_radius_batch.py compares the arrays with the Python mirror's.
program radius_batch_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n_clouds, n, dim, loops
  real(c_float) :: radius
  integer(c_int32_t), allocatable :: offsets(:)
  real(c_float), allocatable :: points(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:)
  real(c_float), allocatable, target :: coords(:,:)
  integer(c_int64_t), allocatable, target :: edge_offsets(:)
  integer(c_int64_t) :: nnz, pairs

  if(command_argument_count() .lt. 2) stop "usage: radius_batch_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_clouds, n, dim, loops
  read(unit) radius
  allocate(offsets(n_clouds + 1), points(dim, n), edge_offsets(n_clouds + 1))
  read(unit) offsets
  read(unit) points
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_radius_graph_batched_host(n_clouds, n, offsets, dim, points, radius, loops, c_null_ptr, c_null_ptr, &
       0_c_int64_t, nnz, c_null_ptr, 0_c_int64_t, pairs, c_null_ptr), "radius_graph_batched_host (size query)")
  allocate(adj_ia(n + 1), adj_ja(2, nnz), coords(dim, pairs))
  call must(athena_mp_radius_graph_batched_host(n_clouds, n, offsets, dim, points, radius, loops, c_loc(adj_ia), c_loc(adj_ja), &
       nnz, nnz, c_loc(coords), pairs, pairs, c_loc(edge_offsets)), "radius_graph_batched_host")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) n_clouds, n, dim, int(nnz, c_int32_t), int(pairs, c_int32_t)
  write(unit) adj_ia, adj_ja, coords, edge_offsets
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "radius graphs: ", n_clouds, " clouds, ", n, " points, ", pairs, " pairs, ", nnz, " entries"
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
end program radius_batch_run
