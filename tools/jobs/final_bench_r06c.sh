mkdir -p results/r06c
( time python bench.py --full --gpus 1 --steps 20 --warmup 5 --detail results/r06c/bench_detail_final.json ) > results/r06c/bench_steps20_warmup5.json 2> results/r06c/bench_final.err
tail -3 results/r06c/bench_final.err; wc -c results/r06c/bench_steps20_warmup5.json
