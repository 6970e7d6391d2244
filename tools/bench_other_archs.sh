# The bench line of every other architecture of the reference's factory (each with its roofline), then the headline's full line,
# into OUT (default: profiles_out/ at the repository root):  bash tools/bench_other_archs.sh
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd $ROOT
O=${OUT:-$ROOT/profiles_out}
mkdir -p $O
for w in cycleaegan cycleae cyclevae doubleae doublevae aegan vaegan; do
  python bench.py --full --workload $w --steps 10 --warmup 3 --no-cpu-baseline >> $O/bench_others.jsonl 2>> $O/bench_others.err || echo "FAILED $w"
done
python bench.py --full --steps 10 --warmup 3 > $O/bench32.json 2> $O/bench32.err
echo done
