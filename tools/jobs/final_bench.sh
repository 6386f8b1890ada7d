mkdir -p results/r06
( time python bench.py --full --gpus 1 --steps 20 --warmup 5 --detail results/r06/bench_detail_final.json ) > results/r06/bench_steps20_warmup5.json 2> results/r06/bench_final.err
tail -4 results/r06/bench_final.err; wc -c results/r06/bench_steps20_warmup5.json
bash tools/profile_round.sh results/r06prof_c4 c4 > results/r06prof_c4.log 2>&1
tail -2 results/r06prof_c4.log
( timeout 300 python tools/sweep_L.py 32 1000000 funnel ) > results/r06/sweep_L_c4.txt 2>&1
( timeout 300 python tools/sweep_L.py 512 100000 iso ) > results/r06/sweep_L_c2.txt 2>&1
cat results/r06/sweep_L_c4.txt results/r06/sweep_L_c2.txt
