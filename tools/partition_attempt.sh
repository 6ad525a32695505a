#!/bin/bash
# One attempt at N > 1 ranks over RCCL on the ONE leased MI355X: in CPX (DPX) compute-partition mode the chip exposes
# 8 (2) HIP devices, which RCCL treats as distinct ranks.  What this could prove: the halo exchange bit for bit across
# real device boundaries, zonal counts exact after the all-reduce, OverlappedHalo under real asynchrony.  What it can NOT
# give: a scaling curve (the partitions share the HBM stacks and have 32 CUs each).
#   gpurun --timeout 900 -- 'bash tools/partition_attempt.sh r06'
# Everything is logged to gpurun_out/<tag>/partition_attempt.log.  READ-ONLY since the pool refused the mode change.
TAG=${1:-r06}
OUT=gpurun_out/$TAG
mkdir -p $OUT
LOG=$OUT/partition_attempt.log
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
ndev() { timeout 60 python - <<'EOF'
import ctypes
hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
n = ctypes.c_int(0)
rc = hip.hipGetDeviceCount(ctypes.byref(n))
print(n.value if rc == 0 else -rc)
EOF
}
{
  echo "== $(date -u) partition attempt, tag $TAG"
  echo "== before: compute / memory partition"
  timeout 60 rocm-smi --showcomputepartition --showmemorypartition 2>&1
  timeout 60 amd-smi partition --current 2>&1 | head -30
  echo "HIP devices before: $(ndev)"
  # (changing the mode is not possible on this pool: gpurun refuses any job that would -- profiles/r06/partition_attempt.log.
  #  What is left: report the mode, and run the multi-device checks if the lease happens to expose more than one device.)
  GOT=""
  [ "$(ndev)" -gt 1 ] 2>/dev/null && GOT=as-leased
  if [ -z "$GOT" ]; then
    echo "== RESULT: one HIP device in this lease; N > 1 over RCCL stays unmeasured on this pool"
  else
    N=$(ndev)
    echo "== RESULT: $GOT holds, $N HIP devices"
    timeout 60 rocm-smi --showcomputepartition 2>&1
    for g in 2 4 8; do
      [ $g -le $N ] || continue
      echo "== bench.py --gpus $g --dry-rccl"
      timeout 240 python -m torch.distributed.run --nnodes=1 --nproc-per-node $g --master-addr 127.0.0.1 --master-port $((29500 + g)) \
        bench.py --gpus $g --dry-rccl 2>&1 | tail -30
      for wl in headline s64 zonal32k; do
        extra=""; [ $wl = s64 ] && extra="--s64-size 16384"; [ $wl = zonal32k ] && extra="--zonal-size 16384"
        echo "== bench.py --gpus $g --workload $wl $extra  (partitions of ONE chip: not a scaling curve)"
        timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node $g --master-addr 127.0.0.1 --master-port $((29600 + g)) \
          bench.py --gpus $g --workload $wl $extra --steps 10 --warmup 3 --full --no-cpu-baseline --no-extras 2>&1 | tail -5
      done
    done
    for g in 2 3 8; do
      [ $g -le $N ] || continue
      echo "== public API on $g row shards, halo rows and zonal partials over RCCL (tools/sharded_rccl_check.py)"
      timeout 400 python tools/sharded_rccl_check.py $g 2>&1 | tail -25
    done
  fi
  echo "HIP devices at exit: $(ndev)"
  timeout 60 rocm-smi --showcomputepartition 2>&1
} > $LOG 2>&1
tail -60 $LOG
