cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out/orth
O=${OUT:-out/orth}; mkdir -p $O
for o in local full periodic selective; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --orth $o --steps 15 > $O/$o.json 2> $O/$o.err || exit 1
  python -c "import json;d=json.load(open('$O/$o.json'));print('$o', round(d['value'],1), d['ms_per_step'], d['kernel_ms_per_step'], d['reorth_passes'])"
done
