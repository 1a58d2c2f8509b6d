#!/bin/bash
# Build the column-chunked form of the joined logreg kernel (gs_logreg_chunked.hip.txt) as a library of its own next to the
# product library's objects, and print the compiler's resource report of both forms.
#   bash benchmarks/variants/build_logreg_chunked.sh [-DLRC_CH=128]   ->  benchmarks/variants/_lib/libgs_logreg_chunked.so
# python benchmarks/bench_eval.py --joined --chunked_lib <that path> then times the two forms in one process.
set -e
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$R/benchmarks/variants/_lib
mkdir -p $OUT
python -m graphsage_amd.build > /dev/null
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-variable -ffp-contract=fast -fno-finite-math-only"
cp $R/benchmarks/variants/gs_logreg_chunked.hip.txt $OUT/gs_logreg_chunked.hip
/opt/rocm/bin/hipcc $FLAGS "$@" -I$R/graphsage_amd/csrc -Rpass-analysis=kernel-resource-usage -c $OUT/gs_logreg_chunked.hip \
  -o $OUT/gs_logreg_chunked.o 2> $OUT/chunked_resources.txt
/opt/rocm/bin/hipcc $FLAGS -Rpass-analysis=kernel-resource-usage -c $R/graphsage_amd/csrc/gs_logreg.hip -o $OUT/gs_logreg_report.o \
  2> $OUT/library_resources.txt
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $OUT/libgs_logreg_chunked.so $R/graphsage_amd/_C/*.o $OUT/gs_logreg_chunked.o
rm -f $OUT/gs_logreg_chunked.o $OUT/gs_logreg_report.o $OUT/gs_logreg_chunked.hip
for f in chunked_resources.txt library_resources.txt; do
  echo "== $f"
  grep -E "Function Name|VGPRs:|AGPRs|Spill|Occupancy|LDS Size|ScratchSize" $OUT/$f | grep -A6 -E "logreg_(joined_)?(chunked_)?kernel" || true
done
echo $OUT/libgs_logreg_chunked.so
