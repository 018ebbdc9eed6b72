!! Top-k vertex selection and its gated rows from FORTRAN through the C ABI: what a caller that holds Fortran arrays does to coarsen
!! a batch of graphs by scores -- select, take the kept rows times the gate, and carry a gradient back.
!!
!!   topk_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_graphs, n, has_k_each, k, has_min_score, F, has_gate; real32 min_score; int32 offsets(n_graphs + 1);
!!                       real32 score(n); with has_k_each = 1: int32 k_each(n_graphs); real32 x(F, n); with has_gate = 1: real32
!!                       gate(n); real32 dy(F, m), m = what the selection keeps
!! result file (stream): int64 m; int32 cluster(n), selected(m), order(m), sel_offsets(n_graphs + 1); real32 y(F, m), dx(F, n),
!!                       dgate(n); int64 stats(4)
!! tests/test_gpu_topk.py compares the arrays with the device entries'.
program topk_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n_graphs, n, has_k_each, k, has_min_score, F, has_gate, g, m32
  real(c_float) :: min_score
  integer(c_int64_t) :: m, room
  integer(c_int32_t), allocatable :: offsets(:)
  integer(c_int32_t), allocatable, target :: k_each(:), cluster(:), selected(:), order(:), sel_offsets(:)
  real(c_float), allocatable :: score(:), dy(:,:), y(:,:)
  real(c_float), allocatable, target :: x(:,:), gate(:), dx(:,:), dgate(:)
  integer(c_int64_t) :: stats(4)
  type(c_ptr) :: k_ptr, gate_ptr

  if(command_argument_count() .lt. 2) stop "usage: topk_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_graphs, n, has_k_each, k, has_min_score, F, has_gate, min_score
  allocate(offsets(n_graphs + 1), score(n), x(F, n))
  read(unit) offsets
  read(unit) score
  k_ptr = c_null_ptr; gate_ptr = c_null_ptr
  if(has_k_each .eq. 1)then
     allocate(k_each(n_graphs))
     read(unit) k_each
     k_ptr = c_loc(k_each)
  end if
  read(unit) x
  if(has_gate .eq. 1)then
     allocate(gate(n))
     read(unit) gate
     gate_ptr = c_loc(gate)
  end if
  ! what selected and order must hold: the sum of min(k_g, n_g)
  room = 0
  do g = 1, n_graphs
     if(has_k_each .eq. 1)then
        room = room + min(k_each(g), offsets(g + 1) - offsets(g))
     else
        room = room + min(k, offsets(g + 1) - offsets(g))
     end if
  end do
  allocate(cluster(n), selected(room), order(room), sel_offsets(n_graphs + 1))

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_topk_vertices_host(n_graphs, n, offsets, score, k, k_ptr, has_min_score, min_score, c_loc(cluster), &
       c_loc(selected), c_loc(order), c_loc(sel_offsets), m), "topk_vertices_host")
  call must(athena_mp_topk_stats(stats), "topk_stats")
  if(m .ne. sel_offsets(n_graphs + 1)) stop "the count is not where the offsets end"
  m32 = int(m, c_int32_t)
  allocate(dy(F, m), y(F, m), dx(F, n), dgate(n))
  read(unit) dy
  close(unit)
  call must(athena_mp_select_rows_host(n, m32, F, selected, x, gate_ptr, y), "select_rows_host")
  call must(athena_mp_select_rows_bwd_host(n, m32, F, cluster, dy, c_loc(x), gate_ptr, c_loc(dx), c_loc(dgate)), &
       "select_rows_bwd_host")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) m, cluster, selected(1:m), order(1:m), sel_offsets, y, dx, dgate, stats
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A)') "selection: ", n, " vertices in ", n_graphs, " graphs, ", m, " kept"
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
end program topk_run
