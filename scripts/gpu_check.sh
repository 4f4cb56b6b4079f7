# GPU validation: parity tests, smoke, the bench line (--full: with its parity check and side workloads; + row-sharded at N = 1)
mkdir -p out
(timeout 1500 python -m pytest tests -q -m gpu 2>&1 | tail -40) > out/pytest_gpu.log
(timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5) > out/smoke.log
(timeout 600 python bench.py --full --steps 50 --warmup 5 2>&1 | tail -1) > out/bench.log
(timeout 600 python bench.py --workload rowshard --steps 2 2>&1 | tail -1) > out/bench_rowshard.log
cat out/pytest_gpu.log out/smoke.log out/bench.log out/bench_rowshard.log
