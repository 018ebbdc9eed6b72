!! A mini-batch out of a dataset graph from FORTRAN through the C ABI: take the handle of a CSR (athena_mp_graph_acquire), make
!! the batch plan (athena_mp_batch_plan_create), select structures (athena_mp_batch_select) and write the child's arrays
!! (athena_mp_graph_export) and the two index maps (athena_mp_memcpy_d2h) to a file.
!!
!!   batch_select_run <case-file> <result-file>
!!
!! case file (stream):   int32 n, nnz, n_edge_cols, n_structures, n_sel; int32 adj_ia(n + 1), adj_ja(2, nnz);
!!                       int32 offsets(n_structures + 1); int64 edge_offsets(n_structures + 1) when n_edge_cols > 0;
!!                       int32 sel(n_sel)                                  (offsets and sel 0-based, as the C ABI takes them)
!! result file (stream): int32 n_child, ne_child; for which = 0 .. 12: int32 count, then count 4-byte elements;
!!                       int32 offsets_out(n_sel + 1); int64 edge_offsets_out(n_sel + 1); int32 vertex_map(n_child), edge_map(ne_child)
!! tests/test_gpu_batch_select.py compares the arrays with the Python mirror's.
program batch_select_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n, nnz32, n_edge_cols, nb, n_sel, which, n_child, ne_child
  integer(c_int32_t), allocatable :: adj_ia(:), adj_ja(:,:), offsets(:), sel(:)
  integer(c_int64_t), allocatable, target :: edge_offsets(:), edge_offsets_out(:)
  integer(c_int32_t), allocatable, target :: offsets_out(:), buf(:), vertex_map(:), edge_map(:)
  integer(c_int64_t) :: count
  type(c_ptr) :: graph, plan, p_eoff, d_vmap, d_emap
  type(c_ptr), target :: child

  if(command_argument_count() .lt. 2) stop "usage: batch_select_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n, nnz32, n_edge_cols, nb, n_sel
  allocate(adj_ia(n + 1), adj_ja(2, nnz32), offsets(nb + 1), edge_offsets(nb + 1), sel(n_sel))
  read(unit) adj_ia
  read(unit) adj_ja
  read(unit) offsets
  if(n_edge_cols .gt. 0) read(unit) edge_offsets
  read(unit) sel
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_graph_acquire(n, int(nnz32, c_int64_t), adj_ia, adj_ja, n_edge_cols, graph), "graph_acquire")
  p_eoff = c_null_ptr
  if(n_edge_cols .gt. 0) p_eoff = c_loc(edge_offsets)
  call must(athena_mp_batch_plan_create(graph, nb, offsets, p_eoff, plan), "batch_plan_create")
  allocate(offsets_out(n_sel + 1), edge_offsets_out(n_sel + 1))
  ! size query first: the maps are allocated from what it returns
  call must(athena_mp_batch_select(plan, n_sel, sel, c_null_ptr, c_loc(offsets_out), c_loc(edge_offsets_out), c_null_ptr, &
       c_null_ptr), "batch_select (size query)")
  n_child = offsets_out(n_sel + 1)
  ne_child = int(edge_offsets_out(n_sel + 1), c_int32_t)
  call must(athena_mp_malloc(d_vmap, 4_c_int64_t * max(n_child, 1)), "malloc")
  call must(athena_mp_malloc(d_emap, 4_c_int64_t * max(ne_child, 1)), "malloc")
  call must(athena_mp_batch_select(plan, n_sel, sel, c_loc(child), c_loc(offsets_out), c_loc(edge_offsets_out), d_vmap, d_emap), &
       "batch_select")
  ! the child is independent: the plan and the dataset handle go first
  call must(athena_mp_batch_plan_destroy(plan), "batch_plan_destroy")
  call must(athena_mp_graph_release(graph), "graph_release")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) n_child, ne_child
  do which = 0, 12
     call must(athena_mp_graph_export(child, which, c_null_ptr, 0_c_int64_t, count), "graph_export (size query)")
     allocate(buf(max(count, 1_c_int64_t)))
     call must(athena_mp_graph_export(child, which, c_loc(buf), count, count), "graph_export")
     write(unit) int(count, c_int32_t)
     write(unit) buf(1:count)
     deallocate(buf)
  end do
  allocate(vertex_map(max(n_child, 1)), edge_map(max(ne_child, 1)))
  if(n_child .gt. 0) call must(athena_mp_memcpy_d2h(vertex_map, d_vmap, 4_c_int64_t * n_child), "memcpy_d2h")
  if(ne_child .gt. 0) call must(athena_mp_memcpy_d2h(edge_map, d_emap, 4_c_int64_t * ne_child), "memcpy_d2h")
  write(unit) offsets_out, edge_offsets_out
  write(unit) vertex_map(1:n_child), edge_map(1:ne_child)
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A)') "batch: ", n_sel, " structures, ", n_child, " vertices, ", ne_child, " edge columns"
  call must(athena_mp_free(d_vmap), "free")
  call must(athena_mp_free(d_emap), "free")
  call must(athena_mp_graph_destroy(child), "graph_destroy")
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
end program batch_select_run
