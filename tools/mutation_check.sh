#!/bin/bash
# Does a test notice when the multi-sequence walk of the large-batch kernels is broken?  (round-2 VERDICT: "Done = a test
# fails if `recn` / `p = pn` (scone_embed_wave.h) is broken on purpose".)
#
#   tools/mutation_check.sh build                       (no GPU needed: hipcc cross-compiles the mutants into build/mutants/)
#   tools/mutation_check.sh run [outdir] [mutant ...]   (on an MI355X: runs the tests against the unmodified library and each
#                                                        mutant; default: every mutant, output in build/mutation/)
#
# Mutants (copies of scone_amd/csrc under build/ with one line changed; the product sources are never touched).  Every one
# stays IN BOUNDS by construction: it only reads or writes addresses the unmodified kernel also touches in the same launch.
#   stale_record    k_embed_wave: the prefetched record of the wave's next token is taken over except for its first id
#   skip_sequence   k_embed_wave: the walk advances by two sequences instead of one
#   stale_position  k_embed_wave: the carried position id is never refreshed (`posv = posn;` dropped)
#   any_no_advance  k_embed_wave_any: the token index is computed from b0 instead of b
#   stale_count     both kernels, partial-sum form: counts[p] gets the hit count of the run's FIRST token
# Expected:
#   stale_record, skip_sequence     tests/test_gpu_bench_shape.py FAILS; the small-batch parity suites (one sequence per
#                                   workgroup: the loop body runs once) cannot see either
#   stale_position, any_no_advance, stale_count
#                                   tests/test_gpu_walk_shapes.py FAILS; the many-sequence tests that existed before it
#                                   (bench shape: default positions, d = 768; parity: shape sweep below the launch target,
#                                   high-occupancy test with arange positions) still PASS
# Every GPU step runs under its own time limit.  A step that ends with anything but pytest's "all passed" (0) or "some
# tests failed" (1) -- an abort, a signal, a timeout, a collection error -- stops the script: nothing more is started.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/scone_amd/csrc
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function -Wno-pass-failed -Wno-unused-variable"
OLD_MUTANTS="stale_record skip_sequence"
NEW_MUTANTS="stale_position any_no_advance stale_count"
M=$R/build/mutants  # the mutant libraries
mutate() {  # name, sed expression on scone_embed_wave.h
  local name=$1 expr=$2 B=$R/build/mut_$1
  rm -rf $B && mkdir -p $B/csrc $M
  cp $C/*.h $C/scone_gather*.hip $B/csrc/
  mkdir -p $B/include && cp $R/include/*.h $B/include/
  sed -i "s#\.\./\.\./include/#../include/#" $B/csrc/*.h $B/csrc/*.hip
  sed -i "$expr" $B/csrc/scone_embed_wave.h
  if diff -q $C/scone_embed_wave.h $B/csrc/scone_embed_wave.h > /dev/null; then echo "mutation $name did not apply"; exit 1; fi
  echo "-- $name:"; diff $C/scone_embed_wave.h $B/csrc/scone_embed_wave.h
  pids=()
  for f in scone_gather_f32 scone_gather_f16 scone_gather_i8 scone_gather_i4 scone_gather; do
    ( cd $B/csrc && hipcc $FLAGS -c $f.hip -o $B/$f.o ) & pids+=($!)
  done
  for p in "${pids[@]}"; do wait $p || exit 1; done
  hipcc -shared --offload-arch=gfx950 -o $M/libmut_$name.so $B/*.o $C/scone_api.o $C/scone_index.o $C/scone_table.o \
    $C/scone_fit.o $C/scone_stage.o $C/scone_shard.o $C/scone_ipc.o || exit 1
  echo "built build/mutants/libmut_$name.so"
}
case ${1:-} in
build)
  make -C $C -j8 > /dev/null || exit 1
  # in bounds: rec[0] keeps an id the same wave loaded (and range-checked by the match) for an earlier token of its walk
  mutate stale_record 's|for (int j = 0; j < W; ++j) rec\[j\] = recn\[j\];|for (int j = 1; j < W; ++j) rec[j] = recn[j];|'
  # in bounds: `more = pn < p_end` still guards every access; only tokens of the run's own sequences are visited
  mutate skip_sequence 's|const long long pn = p + q.T;|const long long pn = p + 2 * (long long)q.T;|'
  # in bounds: posv stays pos[p] of the run's first token, which is range-checked before every use like any other
  # position id; the wpe row read is one the unmodified kernel reads for that first token
  mutate stale_position 's|^    posv = posn;$||'
  # in bounds: p is the run's first token in every iteration -- the records, token / position ids and the output row of a
  # token the unmodified kernel visits too; the other tokens of the run are simply never written
  mutate any_no_advance 's|const long long p = (long long)b \* q.T + i;|const long long p = (long long)b0 * q.T + i;|'
  # in bounds: the extra read is word W - 2 of the record of the run's first token, which the unmodified kernel loads itself
  mutate stale_count 's|if (lane == 0) counts\[p\] = kfull;|if (lane == 0) counts[p] = ell[((long long)b0 * q.T + i) * W + W - 2] >> 8;|'
  ;;
run)
  O=${2:-$R/build/mutation}
  case $O in /*) ;; *) O=$PWD/$O;; esac
  shift; [ $# -gt 0 ] && shift
  MUTANTS=${*:-$OLD_MUTANTS $NEW_MUTANTS}
  mkdir -p $O
  cd $R
  verdict=0
  step() {  # label, expected outcome (pass | fail), time limit in seconds, library ("" = the unmodified one), pytest arguments
    local label=$1 expect=$2 secs=$3 lib=$4 rc; shift 4
    local log=$O/$(echo "$label" | tr -c 'A-Za-z0-9\n' '_').log
    echo "== $label -- must $expect"
    if [ -n "$lib" ]; then SCONE_HIP_LIB=$lib timeout -k 10 $secs python -m pytest "$@" -q > $log 2>&1
    else timeout -k 10 $secs python -m pytest "$@" -q > $log 2>&1; fi
    rc=$?
    grep -E "^(FAILED|ERROR)" $log | cut -c1-200 | head -n 6
    tail -n 1 $log
    case $rc in
      0) if [ $expect = fail ]; then echo "   NOT CAUGHT: the tests passed on this mutant"; verdict=1; fi;;
      1) if [ $expect = pass ]; then echo "   UNEXPECTED: tests failed here"; verdict=1; fi;;
      *) echo "   exit status $rc is no test result (abort, signal, time limit or collection error): stopping"; exit 3;;
    esac
  }
  old_many() {  # the many-sequence tests that existed before tests/test_gpu_walk_shapes.py
    step "$1: bench-shape tests (headline, C2)" $2 900 "$3" tests/test_gpu_bench_shape.py -k "headline or C2"
    step "$1: parity shape sweep + high-occupancy test" $2 900 "$3" tests/test_gpu_parity.py -k "shape_sweep or high_occupancy"
  }
  {
    step "unmodified library: walk shapes" pass 900 "" tests/test_gpu_walk_shapes.py
    old_many "unmodified library" pass ""
    for m in $MUTANTS; do
      L=$M/libmut_$m.so
      [ -f $L ] || { echo "missing $L: run '$0 build' first"; exit 3; }
      case " $OLD_MUTANTS " in
      *" $m "*)
        step "mutant $m: bench-shape tests" fail 900 $L tests/test_gpu_bench_shape.py -k "headline or C2 or eight_shard"
        step "mutant $m: small-batch parity suite (one sequence per workgroup: cannot see it)" pass 600 $L tests/test_gpu_parity.py \
          -k "test_embed_formats_vs_oracle or test_wave_kernel_shape_sweep or test_fused_combine_vs_oracle";;
      *)
        step "mutant $m: walk shapes" fail 900 $L tests/test_gpu_walk_shapes.py
        old_many "mutant $m" pass $L;;
      esac
    done
    echo "== verdict: $([ $verdict = 0 ] && echo "every step ended as expected" || echo "SOME STEP DID NOT END AS EXPECTED")"
    exit $verdict
  } 2>&1 | tee $O/mutation_check.txt
  exit ${PIPESTATUS[0]}
  ;;
*) echo "usage: $0 build | run [outdir] [mutant ...]"; exit 2;;
esac
