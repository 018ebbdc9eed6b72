!! Attention pooling between TWO point sets from FORTRAN through the C ABI, with its reverse steps: what a caller that holds Fortran
!! arrays does for an attention layer over a neighbourhood -- the k-nearest-neighbour graph of the queries in the sources, the
!! handle from that CSR, the softmax of per-edge scores over each query's neighbours, per head, the weighted sum of per-vertex and
!! of per-edge values, and every gradient.
!!
!!   attention_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_queries, n_sources, dim, k, F, H; real32 radius (ieee +infinity: no cap);
!!                       real32 queries(dim, n_queries), sources(dim, n_sources), scores(H, n_queries * k), x(F, n_sources),
!!                       h(F, n_queries * k), dy(F, n_queries)
!!                       (scores and h hold a row for every pair the graph can have; the first `pairs` of them are the edges')
!! result file (stream): int64 pairs; real32 alpha(H, pairs), y_x(F, n_queries), y_h(F, n_queries), dx(F, n_sources),
!!                       dscores_x(H, pairs), dh(F, pairs), dscores_h(H, pairs)
!! tests/test_gpu_attention.py compares the arrays with the device entries' bytes.
program attention_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit, i
  integer(c_int32_t) :: nq, ns, dim, k, F, H
  integer(c_int32_t) :: query_offsets(2), source_offsets(2)
  real(c_float) :: radius
  real(c_float), allocatable :: queries(:,:), sources(:,:), dy(:,:), scores(:,:)
  real(c_float), allocatable, target :: x(:,:), hval(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), row_deg(:), col_deg(:)
  real(c_float), allocatable, target :: coords(:,:), alpha(:,:), y_x(:,:), y_h(:,:), dx(:,:), dh(:,:)
  real(c_float), allocatable, target :: dscores_x(:,:), dscores_h(:,:)
  integer(c_int64_t) :: pairs
  type(c_ptr) :: graph

  if(command_argument_count() .lt. 2) stop "usage: attention_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) nq, ns, dim, k, F, H
  read(unit) radius
  allocate(queries(dim, nq), sources(dim, ns), scores(H, nq * k), x(F, ns), hval(F, nq * k), dy(F, nq))
  read(unit) queries, sources, scores, x, hval, dy
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

  ! the softmax and the weighted sum over the vertices' and over the edges' values, and back
  allocate(alpha(H, pairs), y_x(F, nq), y_h(F, nq), dx(F, ns), dh(F, pairs), dscores_x(H, pairs), dscores_h(H, pairs))
  call must(athena_mp_attention_host(graph, F, H, scores, c_loc(x), c_null_ptr, c_loc(alpha), y_x), "attention_host (x)")
  call must(athena_mp_attention_host(graph, F, H, scores, c_null_ptr, c_loc(hval), c_null_ptr, y_h), "attention_host (h)")
  call must(athena_mp_attention_bwd_host(graph, F, H, alpha, c_loc(x), c_null_ptr, dy, c_loc(dx), c_null_ptr, c_loc(dscores_x)), &
       "attention_bwd_host (x)")
  call must(athena_mp_attention_bwd_host(graph, F, H, alpha, c_null_ptr, c_loc(hval), dy, c_null_ptr, c_loc(dh), c_loc(dscores_h)), &
       "attention_bwd_host (h)")
  call must(athena_mp_graph_destroy(graph), "graph_destroy")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) pairs
  write(unit) alpha, y_x, y_h, dx, dscores_x, dh, dscores_h
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A,I0,A)') "attention: ", nq, " queries, ", ns, " sources, ", pairs, " pairs, ", F, " features, ", H, " heads"
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
end program attention_run
