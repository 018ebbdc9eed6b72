!! The neighbour graphs of a batch of periodic structures from FORTRAN through the C ABI: what a caller that holds Fortran arrays
!! does instead of get_graph_from_basis + generate_adjacency per structure -- query, allocate, fill.
!!
!!   periodic_graph_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_structures, n_atoms, add_self_loops, pbc(3); real32 cutoff_min, cutoff_max;
!!                       int32 offsets(n_structures + 1); real32 frac(3, n_atoms), lat(3, 3, n_structures)
!!                       (lat(c, a, s) = component c of lattice vector a: the row-major [B, 3, 3] array of the C side)
!! result file (stream): int32 n_structures, n_atoms, nnz, pairs; int32 adj_ia(n_atoms + 1), adj_ja(2, nnz);
!!                       real32 feature(pairs), vec(3, pairs); int32 first_count(n_atoms); int64 edge_offsets(n_structures + 1)
!! tests/test_gpu_periodic_graph.py compares the arrays with the Python mirror's.
program periodic_graph_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: nb, n, loops, pbc(3)
  real(c_float) :: cutoff_min, cutoff_max
  integer(c_int32_t), allocatable :: offsets(:)
  real(c_float), allocatable :: frac(:,:), lat(:,:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), first_count(:)
  real(c_float), allocatable, target :: feature(:), vec(:,:)
  integer(c_int64_t), allocatable, target :: edge_offsets(:)
  integer(c_int64_t) :: nnz, pairs

  if(command_argument_count() .lt. 2) stop "usage: periodic_graph_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) nb, n, loops, pbc
  read(unit) cutoff_min, cutoff_max
  allocate(offsets(nb + 1), frac(3, n), lat(3, 3, nb))
  read(unit) offsets
  read(unit) frac
  read(unit) lat
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_periodic_graph_host(nb, n, offsets, frac, lat, pbc, cutoff_min, cutoff_max, loops, c_null_ptr, &
       c_null_ptr, 0_c_int64_t, nnz, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int64_t, pairs, c_null_ptr), &
       "periodic_graph_host (size query)")
  allocate(adj_ia(n + 1), adj_ja(2, nnz), feature(pairs), vec(3, pairs), first_count(n), edge_offsets(nb + 1))
  call must(athena_mp_periodic_graph_host(nb, n, offsets, frac, lat, pbc, cutoff_min, cutoff_max, loops, c_loc(adj_ia), &
       c_loc(adj_ja), nnz, nnz, c_loc(feature), c_loc(vec), c_loc(first_count), pairs, pairs, c_loc(edge_offsets)), &
       "periodic_graph_host")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) nb, n, int(nnz, c_int32_t), int(pairs, c_int32_t)
  write(unit) adj_ia, adj_ja, feature, vec, first_count, edge_offsets
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "periodic graphs: ", nb, " structures, ", n, " atoms, ", pairs, " edges, ", nnz, " entries"
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
end program periodic_graph_run
