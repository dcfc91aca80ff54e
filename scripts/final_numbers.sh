#!/bin/bash
# the numbers quoted in DESIGN.md 7: every BASELINE.json config once
# usage: scripts/final_numbers.sh <outdir>
out=${1:?usage: scripts/final_numbers.sh <outdir>}
mkdir -p $out
python bench.py --full > $out/bench_1080p.json 2> $out/bench_1080p.err && tail -c 600 $out/bench_1080p.json | head -c 0
for w in c2 c1 c5 paraffin_lamp; do
  timeout -k 10 300 python bench.py --workload $w --steps 3 --warmup 1 --no-cpu-baseline > $out/bench_$w.json 2> $out/bench_$w.err || echo "$w failed"
done
timeout -k 10 300 python scripts/time_scene.py diamond 480 270 512 50 > $out/diamond_480.txt 2>&1
timeout -k 10 300 python scripts/time_scene.py many_spheres:5:0 480 270 256 20 > $out/many_spheres_480.txt 2>&1
python - "$out" <<'PY'
import json, glob, sys
for f in sorted(glob.glob(sys.argv[1] + '/bench_*.json')):
    try:
        d = json.loads(open(f).read().strip().splitlines()[-1])
        print(f.split('/')[-1], '%.1f Msamples/s  %.1f ms/step' % (d['value'], d['ms_per_step']), 'cpu', (d.get('cpu_baseline') or {}).get('value'))
    except Exception as e:
        print(f, 'ERR', e)
PY
grep "iter 1" $out/*.txt
