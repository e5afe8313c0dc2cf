"""Attention profile of a split from a checkpoint of train.py --save: per query relation and hop, the edge relations the model
listens to.

    python attn_profile.py --data_path data/family/ --checkpoint family.pt
    python attn_profile.py --ids family_ids.npz --checkpoint family.pt --split valid -k 3 --out profile.tsv

Output (stdout or --out), tab-separated with a header line: query relation, hop, rank, edge relation, mean alpha, alpha sum, edge
count - per query relation that the split asks and per hop the k edge relations with the largest mean alpha over the hop's edges
(RED_GNN_trans.attention_profile).  Relations are names when the dataset has them (relations.txt), ids with --ids; inverse relations
end in '^-1' and the identity relation every entity carries is 'self'.
"""
import argparse
import sys

import numpy as np

from predict import relation_name

HEADER = "query_relation\thop\trank\tedge_relation\tmean_alpha\talpha_sum\tcount"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="RED-GNN attention profile by relation and hop on MI355X")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data_path", type=str, help="dataset directory (entities.txt, relations.txt, facts/train/valid/test.txt)")
    src.add_argument("--ids", type=str, help="npz of id triples (n_ent, n_rel, facts, train, valid, test); output uses ids")
    ap.add_argument("--checkpoint", type=str, required=True, help="file written by train.py --save")
    ap.add_argument("--split", choices=("valid", "test"), default="test")
    ap.add_argument("-k", type=int, default=5, help="edge relations listed per query relation and hop")
    ap.add_argument("--batch", type=int, default=50, help="queries per forward (memory only: the result does not depend on it)")
    ap.add_argument("--max_queries", type=int, default=None, help="only the first so many queries of the split")
    ap.add_argument("--out", type=str, default=None, help="write the table to this file instead of stdout")
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
    if args.k < 1:
        ap.error("-k must be at least 1")
    if args.batch < 1:
        ap.error("--batch must be at least 1")
    return args


def format_profile(prof, n_rel, k=5, id2rel=None):
    """The table as a list of lines (header first) from a group="relation" AttentionProfile: query relations without an edge are
    left out, and a hop lists fewer than k rows where fewer edge relations occur."""
    if prof.group != "relation":
        raise ValueError("format_profile needs a profile grouped by query relation (got group=%r)" % (prof.group,))
    prof = prof.cpu()
    count, asum = prof.count.numpy(), prof.alpha_sum.numpy()
    lines = [HEADER]
    for q in np.nonzero(count.sum((1, 2)) > 0)[0]:
        ids, mean = (t.numpy() for t in prof.top(int(q), k))
        for hop in range(count.shape[1]):
            for rank, (r, m) in enumerate(zip(ids[hop], mean[hop]), 1):
                if r < 0:
                    break
                lines.append("%s\t%d\t%d\t%s\t%.6f\t%.6f\t%d" % (relation_name(int(q), n_rel, id2rel), hop + 1, rank,
                                                                 relation_name(int(r), n_rel, id2rel), m, asum[q, hop, r],
                                                                 count[q, hop, r]))
    return lines


def main(argv=None):
    args = parse_args(argv)

    import torch
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    from red_gnn_amd.profile import split_profile

    torch.cuda.set_device(args.gpu)
    loader = DataLoader(ids=dict(np.load(args.ids)), verbose=False) if args.ids else DataLoader(args.data_path, verbose=False)
    r2i = getattr(loader, "relation2id", None) if not args.ids else None
    id2rel = {v: k for k, v in r2i.items()} if r2i else None

    ckpt = torch.load(args.checkpoint, map_location="cpu")
    o = ckpt["opts"]
    if int(o["n_rel"]) != loader.n_rel or int(o["n_ent"]) != loader.n_ent:
        sys.exit("checkpoint was trained on n_ent=%s n_rel=%s, the data has n_ent=%d n_rel=%d" % (o["n_ent"], o["n_rel"], loader.n_ent,
                                                                                                 loader.n_rel))

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = int(o["n_layer"]), int(o["hidden_dim"]), int(o["attn_dim"]), loader.n_rel, \
            o["act"], float(o.get("dropout", 0.0))

    model = RED_GNN_trans(P, loader).cuda()
    model.load_state_dict(ckpt["state_dict"])
    model.eval()
    prof = split_profile(model, loader, args.split, args.batch, args.max_queries)
    text = "\n".join(format_profile(prof, loader.n_rel, args.k, id2rel)) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
