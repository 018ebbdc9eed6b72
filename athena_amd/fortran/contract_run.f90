!! A pair list contracted over a cluster map from FORTRAN through the C ABI: what a caller that holds Fortran arrays does to
!! coarsen a graph whose connectivity is given (a mesh, a bond list) -- query the two counts, allocate, fill.
!!
!!   contract_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_pairs, n_rows, n_cols, m_rows, m_cols, mode, dim, has_maps, has_points; int32 pairs(2, n_pairs);
!!                       with has_maps = 1: int32 row_cluster(n_rows) and, in mode 1, col_cluster(n_cols);
!!                       with has_points = 1: real32 row_points(dim, m_rows) and, in mode 1, col_points(dim, m_cols)
!!                       (mode 0 is one set: the row arrays serve both sides)
!! result file (stream): int64 P, M; int32 coarse_pairs(2, P), rowptr(P + 1), members(2, M); real32 weights(M); int32
!!                       edge_pair(n_pairs); with has_points = 1: real32 coords(dim, P); int64 stats(4)
!! tests/test_gpu_contract.py compares the arrays with the yardstick's.
program contract_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n_pairs, n_rows, n_cols, m_rows, m_cols, mode, dim, has_maps, has_points
  integer(c_int64_t) :: P, M, P_again, M_again, E
  integer(c_int32_t), allocatable :: pairs(:,:)
  integer(c_int32_t), allocatable, target :: row_cluster(:), col_cluster(:), coarse_pairs(:,:), rowptr(:), members(:,:), edge_pair(:)
  real(c_float), allocatable, target :: row_points(:,:), col_points(:,:), weights(:), coords(:,:)
  integer(c_int64_t) :: stats(4)
  type(c_ptr) :: rc_ptr, cc_ptr, rp_ptr, cp_ptr, coords_ptr

  if(command_argument_count() .lt. 2) stop "usage: contract_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_pairs, n_rows, n_cols, m_rows, m_cols, mode, dim, has_maps, has_points
  allocate(pairs(2, n_pairs))
  read(unit) pairs
  rc_ptr = c_null_ptr; cc_ptr = c_null_ptr; rp_ptr = c_null_ptr; cp_ptr = c_null_ptr; coords_ptr = c_null_ptr
  if(has_maps .eq. 1)then
     allocate(row_cluster(n_rows))
     read(unit) row_cluster
     rc_ptr = c_loc(row_cluster); cc_ptr = rc_ptr
     if(mode .eq. 1)then
        allocate(col_cluster(n_cols))
        read(unit) col_cluster
        cc_ptr = c_loc(col_cluster)
     end if
  end if
  if(has_points .eq. 1)then
     allocate(row_points(dim, m_rows))
     read(unit) row_points
     rp_ptr = c_loc(row_points); cp_ptr = rp_ptr
     if(mode .eq. 1)then
        allocate(col_points(dim, m_cols))
        read(unit) col_points
        cp_ptr = c_loc(col_points)
     end if
  end if
  close(unit)
  E = int(n_pairs, c_int64_t)

  call must(athena_mp_init(0_c_int), "init")
  ! the size query: every output c_null_ptr
  call must(athena_mp_contract_pairs_host(E, pairs, n_rows, n_cols, rc_ptr, cc_ptr, m_rows, m_cols, mode, dim, rp_ptr, cp_ptr, &
       0_c_int64_t, 0_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, P, M), &
       "contract_pairs_host (query)")
  allocate(coarse_pairs(2, P), rowptr(P + 1), members(2, M), weights(M), edge_pair(n_pairs))
  if(has_points .eq. 1)then
     allocate(coords(dim, P))
     coords_ptr = c_loc(coords)
  end if
  call must(athena_mp_contract_pairs_host(E, pairs, n_rows, n_cols, rc_ptr, cc_ptr, m_rows, m_cols, mode, dim, rp_ptr, cp_ptr, &
       P, M, c_loc(coarse_pairs), c_loc(rowptr), c_loc(members), c_loc(weights), c_loc(edge_pair), coords_ptr, P_again, M_again), &
       "contract_pairs_host")
  if(P_again .ne. P .or. M_again .ne. M) stop "the fill found other counts than the query"
  call must(athena_mp_contract_stats(stats), "contract_stats")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) P, M, coarse_pairs, rowptr, members, weights, edge_pair
  if(has_points .eq. 1) write(unit) coords
  write(unit) stats
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A)') "contraction: ", n_pairs, " pairs, ", P, " coarse pairs, ", M, " members"
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
end program contract_run
