R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/build/session}
mkdir -p $OUT; cd $R; export TMPDIR=/tmp
rm -rf $OUT/rp1 $OUT/rp2
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/rp1 -o b -- python $R/bench.py --steps 5 --warmup 2 --full --quick --skip-legs diffquant_wrn,imagenet_resnet18k_dp,nmt_lstm_dp > $OUT/rp1.json 2> $OUT/rp1.err); echo "N=1 under rocprofv3 rc=$? lines=$(wc -l < $OUT/rp1.json)"
python -c "
import json; d=json.loads(open('$OUT/rp1.json').read().strip().splitlines()[-1]); print(d.get('value'), d.get('error'), d.get('bench_process'), d.get('legs_wall_s'))"
grep -v "amdgpu.ids\|simple_timer\|output_stream\|Warning\|warn" $OUT/rp1.err | tail -15 | cut -c1-250
ls $OUT/rp1 | head
(cd /tmp && QD_BENCH_BACKEND=gloo QD_BENCH_ONE_GPU=1 timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/rp2 -o b -- python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 $R/bench.py --gpus 2 --steps 5 --warmup 2 --full --quick --no-cpu-baseline --no-pmc --no-kernels --precondition-s 0.05 --skip-legs diffquant_wrn,nmt_lstm_dp > $OUT/rp2.json 2> $OUT/rp2.err); echo "N=2 gloo under rocprofv3 rc=$? lines=$(wc -l < $OUT/rp2.json)"
grep -v "amdgpu.ids\|simple_timer\|output_stream\|Warning\|warn" $OUT/rp2.err | tail -25 | cut -c1-250
find $OUT/rp1 $OUT/rp2 -name '*.csv' -size +2M -delete
