set -o pipefail
O=${OUT:-build/diag}
mkdir -p "$O"
for L in ${LIBS:-libdnn_hip.so}; do
  n=$(basename $L .so)
  DNN_HIP_LIB=$L timeout -k 10 300 python bench.py --full --kernels --no-cpu --no-latency --no-fp16 --no-unfused --no-e2e --no-fp32-mfma --steps 20 --warmup 3 > "$O/$n.log" 2>&1 || { tail -5 "$O/$n.log"; exit 1; }
  python -c "
import json,sys; d=json.loads(open('$O/$n.log').read().strip().split('\n')[-1]); k=d['kernels']
print('$n', ' '.join('%s %.4f'%(a.split('.')[0],k[a]['ms']) for a in k))"
done
