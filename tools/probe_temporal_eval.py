"""Cost of evaluating one interpolation batch on the ICEWS14-shaped synthetic of BASELINE configs[4] (C5,
synthetic.make_temporal_shape): one JSON line with, per batch of B queries,
  - rg_segment_eval alone, on the logits and (query, entity) pairs of the batch's forward, with both filters;
  - the forward (T_RED_GNN.forward: the dense [B, n_ent] scores) and T_RED_GNN.rank_batch (forward without the dense matrix +
    rg_segment_eval);
  - the reference's way for the same scores (Temporal/interpolation/main.py:142-164), written out in torch on the device: F.softmax
    over [B, n_ent], nll_loss(log(p + 1e-12)), three topk, argsort and one .nonzero().item() per query - raw ranks only;
  - whether the two evaluations agree: logp within rtol 1e-4 / atol 2e-5 of the float64 softmax of the same scores, the batch loss
    within the same of the reference's, and the ranks consistent: the reference's argsort rank + 1 is one of the places of its tie,
    and it sorts fp32 probabilities, where distinct logits far below the row maximum collapse to one value - so the check is that
    [gt + 1, gt + eq + 1] of the logits lies inside the tie interval of the probabilities, which holds the reference's rank; how
    many of the B reference ranks fall inside the logits' own interval is reported next to it.
Times are device-event means over `reps` calls after a warm-up call, taken `rounds` times alternating the contenders (the
reference's Python time lies between its two events); the spread is min..max over rounds.

    python tools/probe_temporal_eval.py C5 64 > profiles/temporal_eval_C5_B64.json
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("cfg", nargs="?", default="C5", help="the temporal shape (C5)")
ap.add_argument("B", nargs="?", type=int, default=64, help="queries per batch")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
if args.cfg != "C5":
    raise SystemExit("probe_temporal_eval: the temporal shape is C5 (got %r)" % args.cfg)

import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import torch.nn.functional as F                                   # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.prediction import temporal_known_index, temporal_static_known_index      # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_temporal_shape     # noqa: E402
from red_gnn_amd.temporal import T_RED_GNN                        # noqa: E402


def mean_ms(f, reps):
    f()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def summary(ts):
    return dict(mean_ms=round(float(np.mean(ts)), 4), min_ms=round(float(np.min(ts)), 4), max_ms=round(float(np.max(ts)), 4))


def reference_way(score, tail):
    """main.py:142-164 and util.py:42-51 on the device: (loss of the batch, hits@1/3/10 counts, argsort ranks)."""
    predicted_prob = F.softmax(score, dim=1)
    loss = F.nll_loss(torch.log(predicted_prob + 1e-12), tail).item()
    hits = [torch.sum(torch.topk(predicted_prob, dim=1, k=k)[1] == tail.unsqueeze(1)).item() for k in (1, 3, 10)]
    sorted_prob = torch.argsort(predicted_prob, dim=-1, descending=True)
    ranks = torch.tensor([sorted_prob[i].eq(tail[i]).nonzero().item() for i in range(len(tail))])
    return loss, hits, ranks


def main():
    torch.cuda.set_device(0)
    B, REPS, ROUNDS = args.B, args.reps, args.rounds
    sh = SHAPES[args.cfg]
    kg = make_temporal_shape(args.cfg)
    quads = kg.quads

    class P:
        pass

    p = P()
    p.n_rel, p.n_ent, p.n_time, p.graph = kg.n_rel, kg.n_ent, kg.n_time, kg.quads
    p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda"
    torch.manual_seed(0)
    model = T_RED_GNN(p).cuda().eval()
    dev = model.linear_classifier.weight.device
    q = np.asarray(quads[:B], dtype=np.int64)
    batch = {"head": q[:, 0], "relation": q[:, 1], "time": q[:, 3]}
    tail = torch.as_tensor(q[:, 2], dtype=torch.int64).to(dev)
    to_dev = lambda ix: tuple(torch.as_tensor(a).to(dev).contiguous() for a in ix)
    known = to_dev(temporal_known_index(quads, kg.n_rel + 1, kg.n_time))
    known_static = to_dev(temporal_static_known_index(quads, kg.n_rel + 1))

    with torch.no_grad():
        score = model(batch, mode="test")
        logits, nodes = model._run(batch, "test", dense=False)
    rb = model.rank_batch(batch, q[:, 2], known, known_static)
    loss, hits, ranks = reference_way(score, tail)
    ranks = ranks.numpy() + 1
    lo, hi = rb.rank("raw", "lo").cpu().numpy(), rb.rank("raw", "hi").cpu().numpy()
    ref_logp = -F.nll_loss(torch.log(F.softmax(score.double(), dim=1) + 1e-12), tail, reduction="none")
    logp_agree = bool(torch.allclose(rb.logp.double(), ref_logp, rtol=1e-4, atol=2e-5))
    loss_agree = bool(abs(-float(rb.logp.double().mean()) - loss) <= 1e-4 * abs(loss) + 2e-5)
    # the reference sorts fp32 PROBABILITIES: logits far below the row maximum underflow to the same probability, so its ties are a
    # superset of the logits' ties and its rank lies in the wider interval [#{p > p_t} + 1, #{p >= p_t}], which must hold the kernel's
    prob = F.softmax(score, dim=1)
    p_t = prob.gather(1, tail.unsqueeze(1))
    lo_p, hi_p = ((prob > p_t).sum(1) + 1).cpu().numpy(), (prob >= p_t).sum(1).cpu().numpy()
    nested = bool(np.all((lo_p <= lo) & (hi <= hi_p)) and np.all((lo_p <= ranks) & (ranks <= hi_p)))
    inside = int(np.sum((lo <= ranks) & (ranks <= hi)))
    same = logp_agree and loss_agree and nested

    seg_ptr = torch.searchsorted(nodes[:, 0].contiguous(), torch.arange(B + 1, dtype=torch.int32, device=dev))
    ent, logits = nodes[:, 1].contiguous(), logits.contiguous()
    target = tail.to(torch.int32)
    key_hr = q[:, 0] * (kg.n_rel + 1) + q[:, 1]
    key_t = torch.as_tensor(key_hr * kg.n_time + q[:, 3], dtype=torch.int64).to(dev)
    key_s = torch.as_tensor(key_hr, dtype=torch.int64).to(dev)
    kernel = [mean_ms(lambda: engine.segment_eval(logits, ent, seg_ptr, target, kg.n_ent, key_t, known, key_s, known_static), 10 * REPS)
              for _ in range(ROUNDS)]
    t = {"forward": [], "rank_batch": [], "reference_way": [], "forward_plus_reference_way": []}
    with torch.no_grad():
        for _ in range(ROUNDS):
            t["forward"].append(mean_ms(lambda: model(batch, mode="test"), REPS))
            t["rank_batch"].append(mean_ms(lambda: model.rank_batch(batch, q[:, 2], known, known_static), REPS))
            t["reference_way"].append(mean_ms(lambda: reference_way(score, tail), REPS))
            t["forward_plus_reference_way"].append(mean_ms(lambda: reference_way(model(batch, mode="test"), tail), REPS))
    lens = (seg_ptr[1:] - seg_ptr[:-1]).cpu().numpy()
    print(json.dumps(dict(
        probe="temporal_eval", cfg=args.cfg, B=B, reps=REPS, rounds=ROUNDS, n_ent=kg.n_ent, n_layer=sh["n_layer"], n_pairs=int(logits.numel()),
        segment_len_mean=round(float(lens.mean()), 1), segment_len_max=int(lens.max()), visited=int(rb.visited.sum()),
        loss=round(-float(rb.logp.double().mean()), 6), reference_loss=round(loss, 6),
        mean_tie_rank_raw=round(float(rb.rank().mean()), 2), mean_tie_rank_fil_t=round(float(rb.rank("fil_t").mean()), 2),
        mean_tie_rank_fil=round(float(rb.rank("fil").mean()), 2), mean_tie_width=round(float((hi - lo).mean()), 1),
        evaluations_agree=same, logp_agree=logp_agree, logp_max_abs_diff=float("%.3g" % float((rb.logp.double() - ref_logp).abs().max())),
        loss_agree=loss_agree, tie_interval_inside_the_probabilities_tie_interval=nested, reference_ranks_inside_tie_interval=inside,
        mean_probability_tie_width=round(float((hi_p - lo_p).mean()), 1), zero_probabilities_per_row=round(float((prob == 0).sum(1).float().mean()), 1),
        rg_segment_eval=summary(kernel), forward=summary(t["forward"]), rank_batch=summary(t["rank_batch"]),
        reference_way=summary(t["reference_way"]), forward_plus_reference_way=summary(t["forward_plus_reference_way"]))))


if __name__ == "__main__":
    main()
