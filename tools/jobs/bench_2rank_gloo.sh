mkdir -p results/r06
( time MJHMC_BENCH_BACKEND=gloo MJHMC_BENCH_ONE_GPU=1 timeout 1500 python bench.py --full --gpus 2 --steps 20 --warmup 5 --workload c4 --no-cpu-baseline --detail results/r06/bench_2rank_detail.json ) > results/r06/bench_2rank_gloo_c4.json 2> results/r06/bench_2rank_gloo_c4.err
tail -5 results/r06/bench_2rank_gloo_c4.err; head -c 1500 results/r06/bench_2rank_gloo_c4.json
