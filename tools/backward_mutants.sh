#!/bin/bash
# Do the backward's GPU tests notice when a kernel of scone_backward.hip is subtly wrong?
#
#   tools/backward_mutants.sh build          (no GPU needed: hipcc cross-compiles the mutants into build/backward_mutants/)
#   tools/backward_mutants.sh run [outdir] [name ...]
#                                            (on an MI355X: both test files against the unmodified library, then against each
#                                            mutant; with names -- "unmodified" or mutants -- only those, appended to the record)
#
# Mutants (copies of scone_amd/csrc under build/ with one statement changed; the product sources are never touched).  Every
# one stays IN BOUNDS by construction: it reads only addresses the unmodified kernel reads in the same launch and writes a
# subset of what that kernel writes (the tests pre-fill what is then left unwritten).  None touches the sort's bit count or a
# capacity formula: those mutants would leave the plan's arrays.
#   tail_dropped          the one-by-one loop of k_bwd_chunks never runs: the last count % 4 references of a chunk are lost
#   neg_zero_start        the accumulators of k_bwd_chunks start at -0.0f
#   second_piece_skipped  on[t] is false for t >= 1: a lane's second to fourth 16-byte piece of a column tile is never summed
#   combine_reversed      k_bwd_combine adds a row's partials last to first
#   stride_once           k_bwd_chunks leaves its chunk loop after one item
#   mean_fused            the mean's multiply and add become one fmaf
# Two columns per library: tests/test_gpu_backward_edges.py (must pass on the unmodified library and FAIL on every mutant, by
# comparison) and tests/test_gpu_backward.py (recorded: what the earlier file alone would have caught).
# A step that ends with anything but pytest's "all passed" (0) or "some tests failed" (1) -- an abort, a signal, a timeout --
# stops the script: nothing more is started.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
M=$R/build/backward_mutants
MUTANTS="tail_dropped neg_zero_start second_piece_skipped combine_reversed stride_once mean_fused"
mutate() {  # name, file, then pairs of (old text, new text): each old text must occur exactly once
  local name=$1 file=$2 B=$R/build/backward_mut_$1
  shift 2
  rm -rf $B && mkdir -p $B/scone_amd $M
  cp -a $R/scone_amd/csrc $B/scone_amd/csrc && cp -a $R/include $B/include || exit 1
  python3 - "$B/scone_amd/csrc/$file" "$@" <<'EOF' || exit 1
import sys
path, pairs = sys.argv[1], sys.argv[2:]
s = open(path).read()
for old, new in zip(pairs[0::2], pairs[1::2]):
    assert s.count(old) == 1, f"mutation does not apply: {old!r} occurs {s.count(old)} times in {path}"
    s = s.replace(old, new)
open(path, "w").write(s)
EOF
  make -C $B/scone_amd/csrc -j8 > $B/make.log 2>&1 || { tail $B/make.log; exit 1; }
  mv $B/scone_amd/csrc/libscone_hip.so $M/libmut_$name.so && echo "built build/backward_mutants/libmut_$name.so"
}
case ${1:-} in
build)
  make -C $R/scone_amd/csrc -j8 > /dev/null || exit 1
  # in bounds: the loop only ever skips loads; the stores after it are the unmodified ones
  mutate tail_dropped scone_backward.hip \
    'for (; i < count; ++i) bwd_walk<DT, NT, MEAN, 1>' \
    'for (; false && i < count; ++i) bwd_walk<DT, NT, MEAN, 1>'
  # in bounds: a constant changes, no address does
  mutate neg_zero_start scone_backward.hip \
    'for (int e = 0; e < E; ++e) acc[t][e] = 0.0f;' \
    'for (int e = 0; e < E; ++e) acc[t][e] = -0.0f;'
  # in bounds: on[t] guards every load and every store of piece t, so fewer of the same loads and stores happen; k_bwd_combine
  # then reads the partial slots it always reads (what was not stored there is whatever the allocation held)
  mutate second_piece_skipped scone_backward.hip \
    'on[t] = tile0 + t * 64 + lane < pieces;' \
    'on[t] = t < 1 && tile0 + t * 64 + lane < pieces;'
  # in bounds: the same mr.n slots of the row, in the other order
  mutate combine_reversed scone_backward.hip \
    'v[r] = *reinterpret_cast<const float4 *>(src + (size_t)(j + r) * d);' \
    'v[r] = *reinterpret_cast<const float4 *>(src + (size_t)(mr.n - 1 - (j + r)) * d);' \
    'const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)j * d);' \
    'const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)(mr.n - 1 - j) * d);'
  # in bounds: a wave does its first chunk as before and no other
  mutate stride_once scone_backward.hip \
    'for (uint32_t ci = wave0; ci < n_chunks; ci += wave_stride) {' \
    'for (uint32_t ci = wave0; ci < n_chunks; ci = n_chunks) {'
  # in bounds: the same operands, one rounding instead of two
  mutate mean_fused scone_backward.hip \
    '          const float cc = MEAN ? f[e] * wr[r] : f[e];
          acc[t][e] = acc[t][e] + cc;' \
    '          acc[t][e] = MEAN ? fmaf(f[e], wr[r], acc[t][e]) : acc[t][e] + f[e];'
  ;;
run)
  O=${2:-$R/build/backward_mutation}
  case $O in /*) ;; *) O=$PWD/$O;; esac
  mkdir -p $O
  cd $R
  shift; [ $# -gt 0 ] && shift
  NAMES=${*:-unmodified $MUTANTS}
  verdict=0
  step() {  # label, test file, expected outcome (pass | fail | any), library ("" = the unmodified one)
    local label=$1 file=$2 expect=$3 lib=$4 rc log=$O/$1.$(basename $2 .py).log
    echo "== $label -- $file -- $([ $expect = any ] && echo recorded || echo "must $expect")"
    if [ -n "$lib" ]; then SCONE_HIP_LIB=$lib timeout -k 10 400 python -m pytest $file -m gpu -q --tb=line > $log 2>&1
    else timeout -k 10 400 python -m pytest $file -m gpu -q --tb=line > $log 2>&1; fi
    rc=$?
    grep -E "^(FAILED|ERROR)" $log | sed -E 's/^FAILED [^:]*::([a-z_0-9]*)(\[.*|$)/\1/' | sort | uniq -c
    tail -n 1 $log
    if grep -qiE "illegal memory access|core dumped|Segmentation fault" $log; then echo "   a fault, not a comparison: stopping"; exit 3; fi
    case $rc in
      0) if [ $expect = fail ]; then echo "   NOT CAUGHT: the tests passed on this mutant"; verdict=1; fi
         if [ $expect = any ]; then echo "   not caught by this file"; fi;;
      1) if [ $expect = pass ]; then echo "   UNEXPECTED: tests failed here"; verdict=1; fi;;
      *) echo "   exit status $rc is no test result (abort, signal, time limit or collection error): stopping"; exit 3;;
    esac
  }
  {
    for m in $NAMES; do
      if [ $m = unmodified ]; then
        step unmodified tests/test_gpu_backward_edges.py pass ""
        step unmodified tests/test_gpu_backward.py pass ""
        continue
      fi
      L=$M/libmut_$m.so
      [ -f $L ] || { echo "missing $L: run '$0 build' first"; exit 3; }
      step $m tests/test_gpu_backward_edges.py fail $L
      step $m tests/test_gpu_backward.py any $L
    done
    echo "== verdict: $([ $verdict = 0 ] && echo "every step ended as expected" || echo "SOME STEP DID NOT END AS EXPECTED")"
    exit $verdict
  } 2>&1 | tee -a $O/backward_mutants.txt
  exit ${PIPESTATUS[0]}
  ;;
*) echo "usage: $0 build | run [outdir]"; exit 2;;
esac
