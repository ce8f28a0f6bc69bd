O=${O:?set O to the output directory}; mkdir -p "$O"
for rep in 1 2; do for p in 0 1; do
for w in aes128 chacha20; do GSC_STREAM_PRIORITIES=$p python bench.py --full --workload $w --batch 1 --callers 1 --steps 40 --warmup 5 --no-cpu-baseline --verify 0 > $O/b1_${w}_p$p.json 2>/dev/null && python3 -c "import json; d=json.load(open('$O/b1_${w}_p$p.json')); print('$w priorities=$p', d['ms_per_step'], {k: round(v,2) for k,v in d['stage_ms_last_step'].items()})"; done; done; done
