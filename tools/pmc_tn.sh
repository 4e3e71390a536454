#!/bin/bash
# HBM bytes of every weight-gradient GEMM shape, per launch.
#   tools/pmc_tn.sh <outdir>   ->  <outdir>/pmc_tn.txt
out=${1:-gpurun_out/pmc_tn}; mkdir -p $out
export TMPDIR=/tmp
: > $out/pmc_tn.txt
rm -rf $out/p
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $out/p -o res -- python3 tools/mb_tn_all.py > $out/p.log 2>&1
python3 tools/rocpd_pmc_dispatch.py $(find $out/p -name "*.db" | head -1) gemm_tn >> $out/pmc_tn.txt 2>&1
grep algorithmic $out/p.log >> $out/pmc_tn.txt
rm -rf $out/p
cat $out/pmc_tn.txt
