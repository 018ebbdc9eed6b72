!! Forces, the fractional gradient, the virial and the cell gradient of a batch of periodic structures from FORTRAN through the
!! C ABI: build the graphs (athena_mp_periodic_graph_host), take the handle of that CSR (athena_mp_graph_acquire) and carry a
!! per-edge gradient back to the atoms and the cell (athena_mp_periodic_grad_host).
!!
!!   geometry_grad_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_structures, n_atoms, add_self_loops, pbc(3), fe_cols, has_dvec; real32 cutoff_min, cutoff_max;
!!                       int32 offsets(n_structures + 1); real32 frac(3, n_atoms), lat(3, 3, n_structures); int32 pairs;
!!                       real32 dfeature(fe_cols, pairs) when fe_cols > 0; real32 dvec(3, pairs) when has_dvec /= 0
!!                       (pairs = the edge count of the batch, which the writer of the gradients knows; it is checked)
!! result file (stream): int32 n_structures, n_atoms, pairs; real32 dcart(3, n_atoms), dfrac(3, n_atoms),
!!                       virial(3, 3, n_structures), dlat(3, 3, n_structures)
!! tests/test_gpu_geometry_grad.py compares the arrays with the Python mirror's.
program geometry_grad_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: nb, n, loops, pbc(3), fe_cols, has_dvec, pairs_in
  real(c_float) :: cutoff_min, cutoff_max
  integer(c_int32_t), allocatable :: offsets(:)
  real(c_float), allocatable :: frac(:,:), lat(:,:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:)
  real(c_float), allocatable, target :: feature(:), vec(:,:), dfeature(:,:), dvec(:,:)
  real(c_float), allocatable, target :: dcart(:,:), dfrac(:,:), virial(:,:,:), dlat(:,:,:)
  integer(c_int64_t), allocatable, target :: edge_offsets(:)
  integer(c_int64_t) :: nnz, pairs
  type(c_ptr) :: graph, p_dfeature, p_dvec

  if(command_argument_count() .lt. 2) stop "usage: geometry_grad_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) nb, n, loops, pbc, fe_cols, has_dvec
  read(unit) cutoff_min, cutoff_max
  allocate(offsets(nb + 1), frac(3, n), lat(3, 3, nb))
  read(unit) offsets
  read(unit) frac
  read(unit) lat
  read(unit) pairs_in
  allocate(dfeature(max(fe_cols, 1), pairs_in), dvec(3, pairs_in))
  if(fe_cols .gt. 0) read(unit) dfeature
  if(has_dvec .ne. 0) read(unit) dvec
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_periodic_graph_host(nb, n, offsets, frac, lat, pbc, cutoff_min, cutoff_max, loops, c_null_ptr, &
       c_null_ptr, 0_c_int64_t, nnz, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int64_t, pairs, c_null_ptr), &
       "periodic_graph_host (size query)")
  if(pairs .ne. int(pairs_in, c_int64_t))then
     write(0,*) "the case file holds gradients of ", pairs_in, " edges, the batch has ", pairs
     stop 1
  end if
  allocate(adj_ia(n + 1), adj_ja(2, nnz), feature(pairs), vec(3, pairs), edge_offsets(nb + 1))
  call must(athena_mp_periodic_graph_host(nb, n, offsets, frac, lat, pbc, cutoff_min, cutoff_max, loops, c_loc(adj_ia), &
       c_loc(adj_ja), nnz, nnz, c_loc(feature), c_loc(vec), c_null_ptr, pairs, pairs, c_loc(edge_offsets)), &
       "periodic_graph_host")
  call must(athena_mp_graph_acquire(n, nnz, adj_ia, adj_ja, int(pairs, c_int32_t), graph), "graph_acquire")

  allocate(dcart(3, n), dfrac(3, n), virial(3, 3, nb), dlat(3, 3, nb))
  p_dfeature = c_null_ptr
  p_dvec = c_null_ptr
  if(fe_cols .gt. 0) p_dfeature = c_loc(dfeature)
  if(has_dvec .ne. 0) p_dvec = c_loc(dvec)
  call must(athena_mp_periodic_grad_host(graph, nb, n, offsets, edge_offsets, lat, cutoff_max, vec, p_dfeature, fe_cols, p_dvec, &
       c_loc(dcart), c_loc(dfrac), c_loc(virial), c_loc(dlat)), "periodic_grad_host")
  call must(athena_mp_graph_release(graph), "graph_release")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) nb, n, int(pairs, c_int32_t)
  write(unit) dcart, dfrac, virial, dlat
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A)') "geometry gradients: ", nb, " structures, ", n, " atoms, ", pairs, " edges"
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
end program geometry_grad_run
