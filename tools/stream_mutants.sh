#!/bin/bash
# Does a test notice when an entry point breaks the stream contract of include/scone_hip.h -- a kernel on stream 0, a hidden
# synchronise, a synchronise of the wrong stream, a cross-stream hop without its wait?  tests/test_gpu_stream_order.py must;
# the tests that existed before it cannot (they call the library with complete inputs on an idle device, where every one of
# these libraries computes the right bits).
#
#   tools/stream_mutants.sh build                       (no GPU needed: hipcc cross-compiles the mutants into build/stream_mutants/)
#   tools/stream_mutants.sh run [outdir] [mutant ...]   (on an MI355X: runs the tests against the unmodified library and against
#                                                        SCONE_HIP_LIB=<mutant>; default: every mutant, output in build/stream_mutation/)
#
# Mutants (copies of scone_amd/csrc under build/ with one line changed; the product sources are never touched).  Each changes
# the ORDERING of one call and nothing else: the same kernel with the same arguments, the same copies, the same addresses.
# The new tests keep every input buffer valid at every moment (their poison is a valid input: ids in range, lists ascending and
# owned, offsets monotone with the same total), so whenever the reordered work runs it stays IN BOUNDS by construction.
#   opt_null_stream             k_opt_step is launched on stream 0 instead of the caller's stream
#   rows_hidden_sync            scone_backward_rows synchronises the caller's stream before it returns (the bits stay right)
#   merge_rows_null_stream      k_grad_merge_rows is launched on stream 0
#   plan_sync_wrong_stream      scone_backward_plan's one synchronise waits for stream 0 instead of the caller's stream
#   leave_no_join               scone_lookup_leave records lookup_out but the caller's stream no longer waits for it
#   upload_reorder_null_stream  the scale reorder kernel behind scone_table_upload's copies is launched on stream 0
# Expected: the unmodified library passes everything; every mutant but one makes tests/test_gpu_stream_order.py FAIL while the
# older tests named beside it below, which exercise the same call, still PASS.
# The one: plan_sync_wrong_stream is EQUIVALENT to the unmodified library under ROCm 7's HIP runtime, and the script expects
# it to pass (measured, profiles/r23a: class S still observes everything queued before the plan completed at return, and U and
# the reference count are right).  The 40-byte hipMemcpyAsync in front of the synchronise copies device memory to PAGEABLE host
# memory on the caller's stream, and the runtime performs such a copy synchronously: it returns after the stream has reached it
# and the bytes have landed.  The synchronise behind it is redundant there; which stream it names cannot be observed.  The
# mutant stays in the list so that a runtime whose pageable copies return early is noticed: the step then fails as "UNEXPECTED",
# which would be the mutant being caught.  (Moving the COPY to stream 0 as well is no admissible mutant: it would read the
# plan's counters before they are written and size launches by uninitialised memory -- out of bounds.)
# leave_no_join is also noticed by one older test, tests/test_gpu_parity.py::test_one_handle_large_batches_from_host_threads
# [own_streams_cu_reserve] (four host threads on their own streams); the older test named for it below is the one written for
# the masked stream, which synchronises around every call and passes.
# Every GPU step runs under its own time limit.  A step that ends with anything but pytest's "all passed" (0) or "some
# tests failed" (1) -- an abort, a signal, a timeout, a collection error -- stops the script: nothing more is started.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/scone_amd/csrc
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function -Wno-pass-failed"
MUTANTS="opt_null_stream rows_hidden_sync merge_rows_null_stream plan_sync_wrong_stream leave_no_join upload_reorder_null_stream"
M=$R/build/stream_mutants  # the mutant libraries
NEW=tests/test_gpu_stream_order.py
older() {  # the older test selection that exercises the mutated call: pytest arguments
  case $1 in
    opt_null_stream) echo "tests/test_gpu_opt_step.py -k kinds_decay";;
    rows_hidden_sync|plan_sync_wrong_stream) echo "tests/test_gpu_backward.py -k cover";;
    merge_rows_null_stream) echo "tests/test_gpu_grad_merge.py";;
    leave_no_join) echo "tests/test_gpu_parity.py -k cu_reserve_runs_the_lookup_on_a_masked_stream";;
    upload_reorder_null_stream) echo "tests/test_gpu_parity.py -k native_table_file_round_trip_against_the_oracle";;
  esac
}
mutate() {  # name, unit (without .hip), sed expression on that unit
  local name=$1 unit=$2 expr=$3 B=$R/build/smut_$1
  local S=$B/scone_amd/csrc  # the tree's own layout: the units include ../../include/scone_hip.h
  rm -rf $B && mkdir -p $S $B/include $M
  cp $C/*.h $C/$unit.hip $S/ && cp $R/include/*.h $B/include/
  sed -i "$expr" $S/$unit.hip
  if diff -q $C/$unit.hip $S/$unit.hip > /dev/null; then echo "mutation $name did not apply"; exit 1; fi
  echo "-- $name:"; diff $C/$unit.hip $S/$unit.hip
  [ "$(diff $C/$unit.hip $S/$unit.hip | grep -c '^>')" = 1 ] || { echo "mutation $name changed more than one line"; exit 1; }
  ( cd $S && hipcc $FLAGS -c $unit.hip -o $B/$unit.o ) || exit 1
  local objs=""
  for o in $C/*.o; do [ "$(basename $o)" = $unit.o ] || objs="$objs $o"; done
  hipcc -shared --offload-arch=gfx950 -o $M/libsmut_$name.so $B/$unit.o $objs || exit 1
  echo "built build/stream_mutants/libsmut_$name.so"
}
case ${1:-} in
build)
  make -C $C -j8 > /dev/null || exit 1
  # in bounds: the same launch with the same arguments; ids and gradient rows are valid whenever it runs (a list that is not
  # ascending or owned would be skipped by the kernel's own id rules anyway)
  mutate opt_null_stream scone_opt 's|dim3(blocks), dim3(256), 0, s, a.ids,$|dim3(blocks), dim3(256), 0, nullptr, a.ids,|'
  # in bounds: nothing is launched differently; the host only waits
  mutate rows_hidden_sync scone_backward '/^extern "C" int scone_backward_rows(/,/^}/ s|^  return SCONE_OK;$|  SCONE_HIP(h, hipStreamSynchronize(s)); return SCONE_OK;|'
  # in bounds: the same launch; every src entry is absent or an index inside its list whenever it runs
  mutate merge_rows_null_stream scone_grad_merge 's|hipLaunchKernelGGL(k_grad_merge_rows, dim3(blocks), dim3(256), 0, (hipStream_t)stream,|hipLaunchKernelGGL(k_grad_merge_rows, dim3(blocks), dim3(256), 0, nullptr,|'
  # in bounds: no launch changes.  The host may read the plan's counts before the copy has landed: they are zero-initialised,
  # an all-zero count is the valid empty plan (U = 0, no partials), and scone_backward_rows refuses (SCONE_ERANGE, nothing
  # written) a caller whose buffers were sized by a U that the landed copy has since replaced
  mutate plan_sync_wrong_stream scone_backward '/hipMemcpyAsync(&pl->m, pl->d_meta, sizeof(bwd_meta)/{n;s|hipStreamSynchronize(s)|hipStreamSynchronize(nullptr)|}'
  # in bounds: the lookup kernel runs on the masked stream with the same arguments; only what FOLLOWS on the caller's stream
  # may now run beside it, and that is the tests' own copies into buffers of unchanged size
  mutate leave_no_join scone_api '/^int scone_lookup_leave(/,/^}/ s|^  if (e == hipSuccess) e = hipStreamWaitEvent(s, h->lookup_out, 0);$|  /* no join */|'
  # in bounds: the reorder kernel permutes the scale slots of rows [row0, row0 + nrows) of the handle's own scales array
  # in place, whichever stream runs it
  mutate upload_reorder_null_stream scone_table 's|scales_reorder_device(h, dst, nrows, 1, s);|scales_reorder_device(h, dst, nrows, 1, nullptr);|'
  ;;
run)
  O=${2:-$R/build/stream_mutation}
  case $O in /*) ;; *) O=$PWD/$O;; esac
  shift; [ $# -gt 0 ] && shift
  CHOSEN=${*:-$MUTANTS}
  mkdir -p $O
  cd $R
  verdict=0
  step() {  # label, expected outcome (pass | fail), time limit in seconds, library ("" = the unmodified one), pytest arguments
    local label=$1 expect=$2 secs=$3 lib=$4 rc; shift 4
    local log=$O/$(echo "$label" | tr -c 'A-Za-z0-9\n' '_').log
    echo "== $label -- must $expect"
    if [ -n "$lib" ]; then SCONE_HIP_LIB=$lib timeout -k 10 $secs python -m pytest "$@" -m gpu -q > $log 2>&1
    else timeout -k 10 $secs python -m pytest "$@" -m gpu -q > $log 2>&1; fi
    rc=$?
    grep -E "^(FAILED|ERROR)" $log | cut -c1-160 | head -n 8
    tail -n 1 $log
    case $rc in
      0) if [ $expect = fail ]; then echo "   NOT CAUGHT: the tests passed on this mutant"; verdict=1; fi;;
      1) if [ $expect = pass ]; then echo "   UNEXPECTED: tests failed here"; verdict=1; fi;;
      *) echo "   exit status $rc is no test result (abort, signal, time limit or collection error): stopping"; exit 3;;
    esac
  }
  {
    step "unmodified library: stream order" pass 300 "" $NEW
    seen=""
    for m in $CHOSEN; do
      case "$seen" in *"|$(older $m)|"*) continue;; esac
      seen="$seen|$(older $m)|"
      step "unmodified library: $(older $m)" pass 300 "" $(older $m)
    done
    for m in $CHOSEN; do
      L=$M/libsmut_$m.so
      [ -f $L ] || { echo "missing $L: run '$0 build' first"; exit 3; }
      if [ $m = plan_sync_wrong_stream ]; then
        step "mutant $m: stream order (EQUIVALENT on this runtime, see the head of the script: nothing can tell it apart)" pass 300 $L $NEW
      else
        step "mutant $m: stream order" fail 300 $L $NEW
      fi
      step "mutant $m: $(older $m) (complete inputs on an idle device: cannot see it)" pass 300 $L $(older $m)
    done
    echo "== verdict: $([ $verdict = 0 ] && echo "every step ended as expected" || echo "SOME STEP DID NOT END AS EXPECTED")"
    exit $verdict
  } 2>&1 | tee $O/stream_mutants.txt
  exit ${PIPESTATUS[0]}
  ;;
*) echo "usage: $0 build | run [outdir] [mutant ...]"; exit 2;;
esac
