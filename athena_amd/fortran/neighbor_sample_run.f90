!! Two hops of neighbour sampling on one graph from FORTRAN through the C ABI: what a caller that holds Fortran arrays does to
!! train on a large graph in mini-batches -- take the handle (athena_mp_graph_acquire), make the sampler plan
!! (athena_mp_sampler_create), then per hop query the sizes, allocate and fill (athena_mp_sample_neighbors_host).  Hop 2's seeds
!! are hop 1's whole vertex_map.
!!
!!   neighbor_sample_run <case-file> <result-file>
!!
!! case file (stream):   int32 n, nnz, n_edge_cols, n_seeds, k(2), degree_mode; int64 seed(2) (the seed of each hop, as the
!!                       definition derives it); int32 adj_ia(n + 1), adj_ja(2, nnz), seeds(n_seeds)        (every id 1-based)
!! result file (stream): per hop: int32 n_cols; int64 nnz; int32 vertex_map(n_cols), entry_map(nnz), edge_map(nnz) (only with
!!                       n_edge_cols > 0), adj_ia(m + 1), adj_ja(2, nnz); then for which = 0 .. 12 of the block's handle: int32
!!                       count and count 4-byte elements.  After both hops: int64 stats(8) of the last one.
!! tests/test_gpu_neighbor_sampling.py compares the arrays with the yardstick's.
program neighbor_sample_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit, hop
  integer(c_int32_t) :: n, nnz32, n_edge_cols, n_seeds, k(2), degree_mode, m, n_cols, n_cols_again, which
  integer(c_int64_t) :: seed(2), nnz, nnz_again, count, stats(8)
  integer(c_int32_t), allocatable :: adj_ia(:), adj_ja(:,:), seeds(:)
  integer(c_int32_t), allocatable, target :: vertex_map(:), entry_map(:), edge_map(:), b_ia(:), b_ja(:,:), buf(:)
  type(c_ptr) :: graph, sampler, p_edge
  type(c_ptr), target :: block

  if(command_argument_count() .lt. 2) stop "usage: neighbor_sample_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n, nnz32, n_edge_cols, n_seeds, k, degree_mode
  read(unit) seed
  allocate(adj_ia(n + 1), adj_ja(2, nnz32), seeds(n_seeds))
  read(unit) adj_ia
  read(unit) adj_ja
  read(unit) seeds
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_graph_acquire(n, int(nnz32, c_int64_t), adj_ia, adj_ja, n_edge_cols, graph), "graph_acquire")
  call must(athena_mp_sampler_create(graph, sampler), "sampler_create")
  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  m = n_seeds
  do hop = 1, 2
     ! the size query: adj_ja = c_null_ptr
     call must(athena_mp_sample_neighbors_host(sampler, m, seeds, k(hop), seed(hop), degree_mode, 0_c_int64_t, 0_c_int64_t, &
          c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, n_cols, nnz, c_null_ptr), "sample_neighbors_host (query)")
     allocate(vertex_map(max(n_cols, 1)), entry_map(max(nnz, 1_c_int64_t)), edge_map(max(nnz, 1_c_int64_t)), b_ia(m + 1), &
          b_ja(2, max(nnz, 1_c_int64_t)))
     p_edge = c_null_ptr
     if(n_edge_cols .gt. 0) p_edge = c_loc(edge_map)
     call must(athena_mp_sample_neighbors_host(sampler, m, seeds, k(hop), seed(hop), degree_mode, int(n_cols, c_int64_t), nnz, &
          c_loc(vertex_map), c_loc(entry_map), p_edge, c_loc(b_ia), c_loc(b_ja), n_cols_again, nnz_again, c_loc(block)), &
          "sample_neighbors_host")
     if(n_cols_again .ne. n_cols .or. nnz_again .ne. nnz) stop "the fill found other sizes than the query"
     write(unit) n_cols, nnz
     write(unit) vertex_map(1:n_cols), entry_map(1:nnz)
     if(n_edge_cols .gt. 0) write(unit) edge_map(1:nnz)
     write(unit) b_ia, b_ja(:, 1:nnz)
     do which = 0, 12
        call must(athena_mp_graph_export(block, which, c_null_ptr, 0_c_int64_t, count), "graph_export (size query)")
        allocate(buf(max(count, 1_c_int64_t)))
        call must(athena_mp_graph_export(block, which, c_loc(buf), count, count), "graph_export")
        write(unit) int(count, c_int32_t)
        write(unit) buf(1:count)
        deallocate(buf)
     end do
     call must(athena_mp_graph_destroy(block), "graph_destroy")
     write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "hop ", hop, ": ", m, " seeds, ", n_cols, " columns, ", nnz, " entries"
     ! the next hop's seeds are this hop's whole vertex_map
     deallocate(seeds)
     allocate(seeds(n_cols))
     seeds = vertex_map(1:n_cols)
     m = n_cols
     deallocate(vertex_map, entry_map, edge_map, b_ia, b_ja)
  end do
  call must(athena_mp_sample_stats(stats), "sample_stats")
  write(unit) stats
  close(unit)
  call must(athena_mp_sampler_destroy(sampler), "sampler_destroy")
  call must(athena_mp_graph_release(graph), "graph_release")
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
end program neighbor_sample_run
