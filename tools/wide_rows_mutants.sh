#!/bin/bash
# Does tests/test_gpu_wide_rows.py notice when a row walk stops short of a wide row?
#
#   tools/wide_rows_mutants.sh build          (no GPU needed: hipcc cross-compiles the mutants into build/wide_mutants/)
#   tools/wide_rows_mutants.sh run [outdir]   (on an MI355X: the file against the unmodified library, then against each mutant)
#
# Mutants (copies of scone_amd/csrc under build/ with one statement changed; the product sources are never touched).  Every
# one stays IN BOUNDS by construction: it reads addresses the unmodified kernel reads in the same launch and writes a subset
# of what that kernel writes (the tests pre-fill what is then left unwritten).
#   stage_copy_one_pass    k_stage_copy copies one 16-bit word of scales per lane and no more (at most 128 bytes per row): the
#                          form this kernel had before tests/test_gpu_wide_rows.py existed
#   units_stop_at_64       embed_units walks the first 64 units of a row only (512 elements)
#   gather_rows_slot0      k_gather_rows takes scale slot 0 for every group of an INT4 / MXFP4 row
#   cols_pack_first_pass   k_cols_pack's scale loop copies only its first pass (lanes_per_rec 16-bit words)
# Expected: the unmodified library passes; every mutant FAILS at least one case, by comparison.
# A step that ends with anything but pytest's "all passed" (0) or "some tests failed" (1) -- an abort, a signal, a timeout --
# stops the script: nothing more is started.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
M=$R/build/wide_mutants
MUTANTS="stage_copy_one_pass units_stop_at_64 gather_rows_slot0 cols_pack_first_pass"
mutate() {  # name, file, then pairs of (old text, new text): each old text must occur exactly once
  local name=$1 file=$2 B=$R/build/wide_mut_$1
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
  cp $B/scone_amd/csrc/libscone_hip.so $M/libmut_$name.so && echo "built build/wide_mutants/libmut_$name.so"
}
case ${1:-} in
build)
  make -C $R/scone_amd/csrc -j8 > /dev/null || exit 1
  # in bounds: a prefix of the words the unmodified loop copies
  mutate stage_copy_one_pass scone_stage.hip \
    'for (unsigned b = lane; b < (unsigned)scale_bytes / 2; b += 64)' \
    'for (unsigned b = lane; b < (unsigned)scale_bytes / 2 && b < 64; b += 64)'
  # in bounds: a prefix of the units the unmodified loop walks; the rest of the output row is never written
  mutate units_stop_at_64 scone_embed_wave.h \
    '  for (int u = (int)lane; u < nu; u += 64) {
    uint32_t raw[KK][RW];' \
    '  for (int u = (int)lane; u < nu && u < 64; u += 64) {
    uint32_t raw[KK][RW];'
  # in bounds: slot 0 of the row's own scales
  mutate gather_rows_slot0 scone_table.hip \
    'const float sf = scone_mx_scale(sc[scone_mx_scale_slot((2 * b) / SCONE_MX_BLOCK, d)]);' \
    'const float sf = scone_mx_scale(sc[scone_mx_scale_slot(0, d)]);' \
    'const float sf = __half2float(scales[lr * ng + scone_i4_scale_slot((2 * b) / SCONE_I4_GROUP, d)]);' \
    'const float sf = __half2float(scales[lr * ng + scone_i4_scale_slot(0, d)]);'
  # in bounds: a prefix of the words the unmodified loop copies
  mutate cols_pack_first_pass scone_shard.hip \
    '      reinterpret_cast<unsigned short *>(scales_out + p * scale_bytes)[b] = reinterpret_cast<const unsigned short *>(scales + lr * scale_bytes)[b];' \
    '      if (b < (unsigned)lanes_per_rec) reinterpret_cast<unsigned short *>(scales_out + p * scale_bytes)[b] = reinterpret_cast<const unsigned short *>(scales + lr * scale_bytes)[b];'
  ;;
run)
  O=${2:-$R/build/wide_mutation}
  case $O in /*) ;; *) O=$PWD/$O;; esac
  mkdir -p $O
  cd $R
  verdict=0
  step() {  # label, expected outcome (pass | fail), library ("" = the unmodified one)
    local label=$1 expect=$2 lib=$3 rc log=$O/$1.log
    echo "== $label -- must $expect"
    if [ -n "$lib" ]; then SCONE_HIP_LIB=$lib timeout -k 10 400 python -m pytest tests/test_gpu_wide_rows.py -m gpu -q --tb=line > $log 2>&1
    else timeout -k 10 400 python -m pytest tests/test_gpu_wide_rows.py -m gpu -q --tb=line > $log 2>&1; fi
    rc=$?
    grep -E "^(FAILED|ERROR)" $log | sed -E 's/^FAILED [^:]*::([a-z_0-9]*)\[.*/\1/' | sort | uniq -c
    tail -n 1 $log
    if grep -qiE "illegal memory access|core dumped|Segmentation fault" $log; then echo "   a fault, not a comparison: stopping"; exit 3; fi
    case $rc in
      0) if [ $expect = fail ]; then echo "   NOT CAUGHT: the tests passed on this mutant"; verdict=1; fi;;
      1) if [ $expect = pass ]; then echo "   UNEXPECTED: tests failed here"; verdict=1; fi;;
      *) echo "   exit status $rc is no test result (abort, signal, time limit or collection error): stopping"; exit 3;;
    esac
  }
  {
    step unmodified pass ""
    for m in $MUTANTS; do
      L=$M/libmut_$m.so
      [ -f $L ] || { echo "missing $L: run '$0 build' first"; exit 3; }
      step $m fail $L
    done
    echo "== verdict: $([ $verdict = 0 ] && echo "every step ended as expected" || echo "SOME STEP DID NOT END AS EXPECTED")"
    exit $verdict
  } 2>&1 | tee $O/wide_rows_mutants.txt
  exit ${PIPESTATUS[0]}
  ;;
*) echo "usage: $0 build | run [outdir]"; exit 2;;
esac
