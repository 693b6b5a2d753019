# multi-rank bench rehearsal on ONE GPU over the host transport (RCCL refuses several ranks
# on one device), in both launch modes the driver may use: torch.distributed.run, and a plain
# `python bench.py --gpus N` (bench.py then starts the rank processes itself).
# usage: tools/bench_rehearsal.sh
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT  # the bench records
for N in 2 4; do
  timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node $N --master-addr 127.0.0.1 --master-port $((29500 + N)) bench.py --full --gpus $N --transport host --grid 256 --steps 5 --warmup 3 > $OUT/rehearsal_$N.json 2> $OUT/rehearsal_$N.err || { tail -20 $OUT/rehearsal_$N.err; exit 1; }
  tail -1 $OUT/rehearsal_$N.json | cut -c1-300
  timeout -k 10 300 python bench.py --full --gpus $N --transport host --grid 256 --steps 5 --warmup 3 > $OUT/rehearsal_plain_$N.json 2> $OUT/rehearsal_plain_$N.err || { tail -20 $OUT/rehearsal_plain_$N.err; exit 1; }
  tail -1 $OUT/rehearsal_plain_$N.json | cut -c1-300
done
