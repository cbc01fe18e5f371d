"""The deployed recurrent weight policy's tick (weight_policy.RecurrentWeightPolicy: ONE launch, csrc/recurrent_policy.h) against the two launches it
fuses -- ``mpc_recurrent_step`` on the actor's memory alone, then ``mpc_policy_step`` on h' with the same actor layers -- at 4096 robots and the
deployment shape (48 observations, 256 state elements, actor 256-512-256-128-12), with the feed-forward ``WeightPolicy.step`` (48-512-256-128-12)
alongside for scale.  One process; the three alternate block by block (the order reverses every block), every launch sits between two events, and a
second pass takes the host clock per block (tools/_rate.py's ``wall_blocks``).

    python tools/policy_rate.py [--robots 4096] [--hidden 256] [--ticks 50] [--blocks 12] [--out profiles/recurrent_policy_rate.json]

The baseline is the composition in the same session.  ``fused_within_composition_spread`` says whether the fused median exceeds the composition's
median by no more than the composition's own p10-p90 spread."""
import argparse

import torch

from _rate import clock, emit, ev, header, stats, wall_blocks      # (puts the repository's root on sys.path)

import rl_mpc_locomotion_amd  # noqa: E402,F401
from rl_mpc_locomotion_amd import recurrent as RC  # noqa: E402
from rl_mpc_locomotion_amd.ppo import ActorCritic  # noqa: E402
from rl_mpc_locomotion_amd.weight_policy import RecurrentWeightPolicy, WeightPolicy, actor_layers  # noqa: E402

ACTOR_HIDDEN = (512, 256, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--obs", type=int, default=48)
    ap.add_argument("--hidden", type=int, default=256, help="the memory's state elements")
    ap.add_argument("--ticks", type=int, default=50, help="launches per block")
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, n, I, H = torch.device("cuda:0"), args.robots, args.obs, args.hidden
    torch.manual_seed(0)
    ac = RC.ActorCriticRecurrent(I, 12, ACTOR_HIDDEN, (16,), rnn_hidden_size=H).to(dev)
    sd = ac.state_dict()
    fused = RecurrentWeightPolicy.from_state_dict(sd, device=dev)
    head = WeightPolicy(actor_layers(sd), device=dev)                            # the same actor layers, reading h'
    torch.manual_seed(1)
    flat = WeightPolicy(actor_layers(ActorCritic(I, 12, ACTOR_HIDDEN, (16,)).state_dict()), device=dev)
    obs = torch.randn(n, I, device=dev)
    reset = torch.zeros(n, dtype=torch.long, device=dev)
    reset[::50] = 1

    def composition():
        h1, = ac.cell_step({RC.ACTOR: obs}, reset)
        return head.step(h1)
    loops = {"fused": lambda: fused.step(obs, reset=reset), "composition": composition, "feed_forward": lambda: flat.step(obs)}
    res = header(args, n, observations=I, hidden_size=H, actor=[H, *ACTOR_HIDDEN, 12], launches_per_tick={"fused": 1, "composition": 2, "feed_forward": 1})
    # the two paths start from the same state and must still agree after the timing (bit for bit: tests/test_recurrent_policy_gpu.py)
    for tick in loops.values():
        for _ in range(20):
            tick()
    fused.reset_memory(); ac.reset_memory()
    torch.cuda.synchronize()
    spans = {k: [] for k in loops}
    names = list(loops)
    for block in range(args.blocks):
        for name in (names if block % 2 == 0 else names[::-1]):
            e = [(ev(), ev()) for _ in range(args.ticks)]
            for a, b in e:
                a.record()
                loops[name]()
                b.record()
            torch.cuda.synchronize()
            spans[name].extend(a.elapsed_time(b) for a, b in e)
    res["equal_after_timing"] = bool(torch.equal(fused.h, ac.memory_a.h) and torch.equal(fused.c, ac.memory_a.c))
    res["launch_ms"] = {k: stats(v) for k, v in spans.items()}
    f, c = res["launch_ms"]["fused"], res["launch_ms"]["composition"]
    res["fused_over_composition_median"] = f["median_ms"] / c["median_ms"]
    res["composition_p10_p90_spread_ms"] = c["p90_ms"] - c["p10_ms"]
    res["fused_minus_composition_median_ms"] = f["median_ms"] - c["median_ms"]
    res["fused_within_composition_spread"] = bool(f["median_ms"] - c["median_ms"] <= c["p90_ms"] - c["p10_ms"])
    res["fused_over_feed_forward_median"] = f["median_ms"] / res["launch_ms"]["feed_forward"]["median_ms"]
    res["wall"] = wall_blocks(loops, args.ticks, args.blocks, n, warmup=0)
    res["wall_fused_over_composition_median"] = res["wall"]["fused"]["ms_per_tick_median"] / res["wall"]["composition"]["ms_per_tick_median"]
    clock(res, "after")
    emit(res, args.out)


if __name__ == "__main__":
    main()
