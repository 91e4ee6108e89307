O=$(mktemp -d)
for m in 0 fwd bwd 1; do
  BP_EPILOGUE_STATS=$m python bench.py --full --legs none --steps 10 --warmup 3 > $O/es_$m.json 2> $O/es_$m.err
  python -c "
import json,sys; d=json.loads(open('$O/es_$m.json').read().strip().splitlines()[-1]); print('$m', d['value'], d['ms_per_step'], d['roofline']['conv_kernels_ms_per_step'])"
done
