!! The edge MLP's input between TWO point sets from FORTRAN through the C ABI, with its reverse: what a caller that holds Fortran
!! arrays does between the graph and the MLP of a set-abstraction step -- the k-nearest-neighbour graph of the coarse points in the
!! fine ones, the handle from that CSR, h(:, e) = (xs(:, j), xq(:, i), coords(:, e)) for every pair e = (i, j), and from the MLP's
!! input gradient dh back to dxs, dxq and dcoords.
!!
!!   edge_gather_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_queries, n_sources, dim, k, Fs, Fq, relative, ld; real32 radius (ieee +infinity: no cap);
!!                       real32 queries(dim, n_queries), sources(dim, n_sources), xs(Fs, n_sources), xq(Fq, n_queries),
!!                       h(ld, n_queries * k), dh(ld, n_queries * k)
!!                       (h and dh hold a column for every pair the graph can have; the first `pairs` of them are used.  h is what
!!                       the output array holds before the call: its elements beyond Fs + Fq + dim must come back unchanged)
!! result file (stream): int64 pairs; real32 h(ld, pairs), dxs(Fs, n_sources), dxq(Fq, n_queries), dcoords(dim, pairs)
!! tests/test_gpu_edge_gather.py compares the arrays with the device entries' bytes.
program edge_gather_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit, i
  integer(c_int32_t) :: nq, ns, dim, k, Fs, Fq, relative, ld
  integer(c_int32_t) :: query_offsets(2), source_offsets(2)
  real(c_float) :: radius
  real(c_float), allocatable :: queries(:,:), sources(:,:), h(:,:), dh(:,:)
  real(c_float), allocatable, target :: xs(:,:), xq(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), row_deg(:), col_deg(:)
  real(c_float), allocatable, target :: coords(:,:), dxs(:,:), dxq(:,:), dcoords(:,:)
  integer(c_int64_t) :: pairs
  type(c_ptr) :: graph, p_xs, p_xq, p_dxs, p_dxq

  if(command_argument_count() .lt. 2) stop "usage: edge_gather_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) nq, ns, dim, k, Fs, Fq, relative, ld
  read(unit) radius
  allocate(queries(dim, nq), sources(dim, ns), xs(Fs, ns), xq(Fq, nq), h(ld, nq * k), dh(ld, nq * k))
  read(unit) queries, sources, xs, xq, h, dh
  close(unit)
  query_offsets = [0_c_int32_t, nq]
  source_offsets = [0_c_int32_t, ns]

  call must(athena_mp_init(0_c_int), "init")
  ! the graph: query, allocate, fill
  call must(athena_mp_knn_graph_bipartite_host(1_c_int32_t, nq, query_offsets, ns, source_offsets, dim, queries, sources, k, radius, &
       c_null_ptr, c_null_ptr, 0_c_int64_t, c_null_ptr, 0_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, pairs), &
       "knn_graph_bipartite_host (size query)")
  allocate(adj_ia(nq + 1), adj_ja(2, pairs), coords(dim, pairs))
  call must(athena_mp_knn_graph_bipartite_host(1_c_int32_t, nq, query_offsets, ns, source_offsets, dim, queries, sources, k, radius, &
       c_loc(adj_ia), c_loc(adj_ja), pairs, c_loc(coords), pairs, c_null_ptr, c_null_ptr, c_null_ptr, pairs), &
       "knn_graph_bipartite_host")
  allocate(row_deg(nq), col_deg(ns))
  row_deg = adj_ia(2:nq + 1) - adj_ia(1:nq)
  col_deg = 0
  do i = 1, int(pairs)
     col_deg(adj_ja(1, i)) = col_deg(adj_ja(1, i)) + 1
  end do
  call must(athena_mp_graph_create(nq, ns, pairs, adj_ia, adj_ja, int(pairs, c_int32_t), c_loc(row_deg), c_loc(col_deg), graph), &
       "graph_create")

  ! the MLP's input, and back from its gradient; a block of width 0 is c_null_ptr
  allocate(dxs(Fs, ns), dxq(Fq, nq), dcoords(dim, pairs))
  p_xs = c_null_ptr; p_xq = c_null_ptr; p_dxs = c_null_ptr; p_dxq = c_null_ptr
  if(Fs .gt. 0)then
     p_xs = c_loc(xs); p_dxs = c_loc(dxs)
  end if
  if(Fq .gt. 0)then
     p_xq = c_loc(xq); p_dxq = c_loc(dxq)
  end if
  call must(athena_mp_edge_gather_host(graph, Fs, p_xs, Fq, p_xq, dim, c_loc(coords), relative, ld, h), "edge_gather_host")
  call must(athena_mp_edge_gather_bwd_host(graph, Fs, Fq, dim, relative, ld, dh, p_dxs, p_dxq, c_loc(dcoords)), &
       "edge_gather_bwd_host")
  call must(athena_mp_graph_destroy(graph), "graph_destroy")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) pairs
  write(unit) h(:, 1:pairs), dxs, dxq, dcoords
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "edge gather: ", nq, " queries, ", ns, " sources, ", pairs, " pairs, ", Fs + Fq + dim, " columns"
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
end program edge_gather_run
