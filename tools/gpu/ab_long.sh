# Same-box A/B of library variants on the long horizons (solver seam): ab_long.sh <name> <name> ...   (two alternating rounds, h = 16 and h = 20, 4096 robots)
cd $GRAFT_REPO_ROOT
for round in 1 2; do
  for v in "$@"; do
    for hc in "16:4" "20:5"; do
      H=${hc%%:*}; C=${hc#*:}
      MPC_LIB_PATH=$PWD/rl-mpc-locomotion_amd/csrc/variants/libmpc_batch_$v.so python bench.py --full --seam solver --config $C --robots 4096 --steps 5 --warmup 3 --repeats 3 --no-secondary --no-cpu-baseline --no-control-loop 2>/dev/null | python -c "
import json,sys; d=json.loads(sys.stdin.read()); print('$v h=$H round $round', round(d['value']), 'solve', round(d['roofline']['kernel_ms'],4), 'prep', round(d['roofline']['prep_kernel_ms'],4), 'iters', round(d['mean_admm_iters'],2), 'solved', d['solved_fraction'])"
    done
  done
done
