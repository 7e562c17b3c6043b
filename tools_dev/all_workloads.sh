# developer helper: one --full bench line per workload into <outdir>/<tag>_<workload>.json (the default chain with its CPU baseline)
O=${1:?outdir}; T=${2:-w}
mkdir -p $O
show() { python -c "
import json,sys;d=json.load(open(sys.argv[1]));r=d.get('roofline') or {}
print(sys.argv[2],'%.4g'%d['value'],'%.4f ms'%d['ms_per_step'],d.get('stage_ms'),r.get('kernel'),r.get('frac'),r.get('traffic'),(r.get('valu_issue') or {}).get('frac'),d.get('whole_step_hbm_frac'),(d.get('parity_checked') or {}).get('max_lsb'),d.get('pcie_inclusive'))" "$1" "$2"; }
python bench.py --full > $O/${T}_chain.json 2> $O/${T}_chain.err; show $O/${T}_chain.json chain
python -c "
import json;d=json.load(open('$O/${T}_chain.json'));print('cpu_baseline',d['cpu_baseline'])"
for w in nsx aecm rtp_chain ns_aec_8k ns_agc_mix_32k ns g711 mfft; do
  python bench.py --workload $w --full --no-cpu > $O/${T}_$w.json 2> $O/${T}_$w.err
  show $O/${T}_$w.json $w
done
for p in 2 4; do
  python bench.py --packets-per-step $p --steps 100 --full --no-cpu > $O/${T}_chain_p$p.json 2>/dev/null; show $O/${T}_chain_p$p.json "chain p$p"
done
