# the round's measurements in one call on the GPU box: the GPU suite, the full bench line, the profiler passes of the legs whose
# kernels or routes changed (summaries only come back: the raw rocprofv3 directories are deleted), the sweeps
# usage: bash tools/lab/r06_run.sh OUTDIR
OUT=${1:?usage: bash tools/lab/r06_run.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q 2>&1 | tail -5 > "$OUT"/pytest_gpu.txt
python bench.py --full > "$OUT"/bench_full.json 2> "$OUT"/bench_full.err
bash tools/prof_all.sh "$OUT"/prof inflate_wg > "$OUT"/prof_all.log 2>&1
python tools/prof_report.py "$OUT"/prof "$OUT"/r06 >> "$OUT"/prof_all.log 2>&1
find "$OUT"/prof -mindepth 1 -maxdepth 1 -type d -exec rm -rf {} +
KERNELS=wg,old SIZES=64,256,1024,4096,16384,65536,131072,262144 python tools/bench_inflate_kernels.py 2>&1 | grep -v amdgpu.ids > "$OUT"/inflate_by_batch_size.txt
SWEEP_KIB=4,16,64,128,256,512,1024,4096,16384 python tools/api_sweep.py > "$OUT"/api_sweep.txt 2>&1
python tools/lab/bench_wg_long.py 2>&1 | grep -v amdgpu.ids > "$OUT"/long_streams.txt
cat "$OUT"/pytest_gpu.txt; du -sh "$OUT"; tail -3 "$OUT"/prof_all.log
