"""Top-k prediction from a checkpoint of train.py --save: the best new answers of queries, optionally with the path behind each.

    python predict.py --data_path data/family/ --checkpoint family.pt -k 5 queries.tsv
    python predict.py --ids family_ids.npz --checkpoint family.pt -k 5 queries.tsv --explain

A query is one line `head<TAB>relation<TAB>?` or `?<TAB>relation<TAB>tail` (the latter is asked as the inverse relation's query
(tail, relation + n_rel, ?)); names go through entities.txt / relations.txt, with --ids they are ids.  Tails the dataset already
holds for the query are left out (RED_GNN_trans.predict, exclude_known=True).  `-` (the default) reads the queries from stdin.
Output: one line per answer, `query<TAB>rank<TAB>entity<TAB>score`, and with --explain the strongest path below it.
"""
import argparse
import sys

import numpy as np


def parse_query(line, n_rel, entity2id=None, relation2id=None):
    """(subject id, relation id) of one query line; ValueError on a malformed line or an unknown name / id.
    Without the name maps (``--ids``) the fields are ids."""
    parts = [p.strip() for p in line.rstrip("\n").split("\t")]
    if len(parts) != 3:
        raise ValueError("query %r: need three tab-separated fields (head, relation, tail), one of them '?'" % line.rstrip("\n"))
    h, r, t = parts
    if (h == "?") == (t == "?"):
        raise ValueError("query %r: exactly one of head and tail must be '?'" % line.rstrip("\n"))

    def lookup(name, table, n, what):
        if table is not None:
            if name not in table:
                raise ValueError("unknown %s %r" % (what, name))
            return int(table[name])
        try:
            v = int(name)
        except ValueError:
            raise ValueError("%s %r is not an id" % (what, name)) from None
        if n is not None and not 0 <= v < n:
            raise ValueError("%s id %d out of range 0..%d" % (what, v, n - 1))
        return v

    rel = lookup(r, relation2id, n_rel, "relation")
    if not 0 <= rel < n_rel:
        raise ValueError("relation id %d out of range 0..%d" % (rel, n_rel - 1))
    if t == "?":
        return lookup(h, entity2id, None, "entity"), rel
    return lookup(t, entity2id, None, "entity"), rel + n_rel


def relation_name(r, n_rel, id2rel=None):
    """Name of a relation id of the doubled vocabulary: r < n_rel as is, inverses with a '^-1', 2*n_rel = the identity 'self'."""
    if r == 2 * n_rel:
        return "self"
    base = r % n_rel
    name = id2rel[base] if id2rel is not None else str(base)
    return name if r < n_rel else name + "^-1"


def main(argv=None):
    ap = argparse.ArgumentParser(description="RED-GNN top-k prediction on MI355X")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data_path", type=str, help="dataset directory (entities.txt, relations.txt, facts/train/valid/test.txt)")
    src.add_argument("--ids", type=str, help="npz of id triples (n_ent, n_rel, facts, train, valid, test); queries and output are ids")
    ap.add_argument("--checkpoint", type=str, required=True, help="file written by train.py --save")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--explain", action="store_true", help="print the strongest path behind each answer")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("queries", nargs="?", default="-", help="file of queries, one per line ('-' = stdin)")
    args = ap.parse_args(argv)

    import torch
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans

    torch.cuda.set_device(args.gpu)
    loader = DataLoader(ids=dict(np.load(args.ids)), verbose=False) if args.ids else DataLoader(args.data_path, verbose=False)
    e2i = getattr(loader, "entity2id", None) if not args.ids else None
    r2i = getattr(loader, "relation2id", None) if not args.ids else None
    id2ent = {v: k for k, v in e2i.items()} if e2i else None
    id2rel = {v: k for k, v in r2i.items()} if r2i else None
    ent_name = (lambda e: id2ent[e]) if id2ent else str

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

    lines = sys.stdin.readlines() if args.queries == "-" else open(args.queries).readlines()
    text, subs, rels = [], [], []
    for ln in lines:
        if not ln.strip():
            continue
        try:
            s, r = parse_query(ln, loader.n_rel, e2i, r2i)
        except ValueError as e:
            sys.exit("predict.py: %s" % e)
        if not 0 <= s < loader.n_ent:
            sys.exit("predict.py: entity id %d out of range 0..%d" % (s, loader.n_ent - 1))
        text.append(ln.strip().replace("\t", " "))
        subs.append(s)
        rels.append(r)
    if not subs:
        return
    pred = model.predict(np.array(subs), np.array(rels), k=args.k)
    ids, sc = pred.ids.cpu().numpy(), pred.scores.cpu().numpy()
    paths = None
    if args.explain:
        rows = np.repeat(np.arange(len(subs)), args.k)
        flat = ids.reshape(-1)
        ok = flat >= 0
        paths = {}
        if ok.any():
            rd = model.explain(np.array(subs)[rows[ok]], np.array(rels)[rows[ok]], flat[ok])
            prel, pent, prod = (t.cpu().numpy() for t in rd.strongest_paths())
            for i, (q, j) in enumerate(zip(rows[ok], np.nonzero(ok)[0] % args.k)):
                paths[(q, j)] = (prel[i], pent[i], prod[i])
    for q in range(len(subs)):
        for j in range(args.k):
            if ids[q, j] < 0:
                break
            print("%s\t%d\t%s\t%.6g" % (text[q], j + 1, ent_name(int(ids[q, j])), sc[q, j]))
            if paths is not None:
                prel, pent, prod = paths[(q, j)]
                if pent[0] < 0:
                    print("\t(no path)")
                    continue
                hops = "".join(" -%s-> %s" % (relation_name(int(r), loader.n_rel, id2rel), ent_name(int(e)))
                               for r, e in zip(prel, pent[1:]))
                print("\tpath %s%s\t(alpha product %.4g)" % (ent_name(int(pent[0])), hops, prod))


if __name__ == "__main__":
    main()
