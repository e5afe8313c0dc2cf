"""CPU checks of the top-k prediction path (-m "not gpu"): the known-answer index against the loaders' filter sets, rg_topk's
argument errors, predict's argument errors without a GPU, and the query parser of predict.py."""
import numpy as np
import pytest
import torch

from tests import _util as U


def _check_index(filters, index, n_rel):
    keys, ptr, idx = index
    assert keys.dtype == np.int64 and ptr.dtype == np.int64 and idx.dtype == np.int32
    assert len(ptr) == len(keys) + 1 and ptr[0] == 0 and ptr[-1] == len(idx)
    assert np.all(np.diff(keys) > 0)
    assert len(keys) == len(filters)
    got = {}
    for i, key in enumerate(keys.tolist()):
        s, r = divmod(key, 2 * n_rel + 1)
        tails = idx[ptr[i]:ptr[i + 1]]
        assert np.all(np.diff(tails) > 0)
        got[(s, r)] = tails.tolist()
    assert got == {k: list(v) for k, v in filters.items()}


@pytest.mark.parametrize("name", ["family_ids.npz", "WN18RR_ids.npz"])
def test_known_index_equals_filters(name):
    from red_gnn_amd.load_data import DataLoader
    loader = DataLoader(ids=U.load(name), verbose=False)
    index = loader.known_index("test")
    _check_index(loader.filters, index, loader.n_rel)
    assert loader.known_index("valid") is index and loader.known_index("train") is index     # one index for every mode, built once


def test_known_index_binary_cache_path(tmp_path):
    """A loader from the binary cache builds the index without the filter dict (which stays unbuilt), and it equals the text path's."""
    from red_gnn_amd.load_data import DataLoader
    ids = U.load("family_ids.npz")
    task = tmp_path / "fam"
    task.mkdir()
    n_ent, n_rel = int(ids["n_ent"]), int(ids["n_rel"])
    (task / "entities.txt").write_text("".join("e%d\n" % i for i in range(n_ent)))
    (task / "relations.txt").write_text("".join("r%d\n" % i for i in range(n_rel)))
    for split, f in (("facts", "facts.txt"), ("train", "train.txt"), ("valid", "valid.txt"), ("test", "test.txt")):
        (task / f).write_text("".join("e%d\tr%d\te%d\n" % tuple(t) for t in ids[split].tolist()))
    cache = str(tmp_path / "cache")
    text = DataLoader(str(task), verbose=False)                           # the text path
    DataLoader(str(task), verbose=False, cache_dir=cache)                 # parses the text and writes the cache
    cached = DataLoader(str(task), verbose=False, cache_dir=cache)        # loads the cache
    assert cached._filters is None
    index = cached.known_index()
    assert cached._filters is None                                         # the per-triple loop did not run
    for a, b in zip(index, text.known_index()):
        assert np.array_equal(a, b)
    _check_index(text.filters, index, n_rel)
    _check_index(cached.filters, index, n_rel)


def test_known_index_inductive_modes():
    from red_gnn_amd.inductive import DataLoader
    loader = DataLoader(ids=U.load("ind_WN18RR_v1_ids.npz"), verbose=False)
    _check_index(loader.val_filters, loader.known_index("transductive"), loader.n_rel)
    _check_index(loader.tst_filters, loader.known_index("inductive"), loader.n_rel)
    assert loader.known_index("train") is loader.known_index("transductive")
    assert loader.known_index("test") is loader.known_index("inductive")


def test_topk_reports_bad_arguments():
    from red_gnn_amd import _lib
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = _lib.ptr(buf)
    ok = (p, 2, 8, 4, p, p, p, p, 1, p, p, None)

    def call(**kw):
        names = ["scores", "batch", "n_ent", "k", "q_key", "keys", "ptr", "idx", "n_keys", "idx_out", "score_out", "stream"]
        a = dict(zip(names, ok))
        a.update(kw)
        return L.rg_topk(*[a[n] for n in names])

    for kw, msg in ((dict(scores=None), b"NULL"), (dict(idx_out=None), b"NULL"), (dict(score_out=None), b"NULL"),
                    (dict(k=0), b"k=0"), (dict(k=1025), b"k=1025"), (dict(k=-1), b"k=-1"),
                    (dict(batch=0), b"batch=0"), (dict(batch=-2), b"batch=-2"), (dict(n_ent=0), b"n_ent=0"), (dict(n_ent=-5), b"n_ent=-5"),
                    (dict(n_keys=-1), b"n_keys=-1"),
                    (dict(q_key=None), b"NULL index"), (dict(keys=None), b"NULL index"), (dict(ptr=None), b"NULL index"),
                    (dict(idx=None), b"NULL index")):
        assert call(**kw) != 0, kw
        assert msg in L.rg_last_error(), (kw, L.rg_last_error())


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_predict_fails_loudly_without_gpu():
    from red_gnn_amd import _lib
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    ids = U.load("tiny_fwd.npz")
    loader = DataLoader(ids=ids, verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = 2, 16, 3, loader.n_rel, "relu", 0.0

    model = RED_GNN_trans(P, loader)
    with pytest.raises(_lib.NativeError):
        model.predict(ids["subs"], ids["rels"], k=3)


def test_predict_query_parser():
    import predict
    e2i = {"alice": 0, "bob": 1, "carol": 2}
    r2i = {"father": 0, "mother": 1}
    assert predict.parse_query("alice\tfather\t?\n", 2, e2i, r2i) == (0, 0)
    assert predict.parse_query("?\tmother\tcarol", 2, e2i, r2i) == (2, 1 + 2)        # (tail, r + n_rel, ?)
    assert predict.parse_query("3\t1\t?", 2) == (3, 1)                                  # ids
    assert predict.parse_query("?\t0\t7", 2) == (7, 2)
    for bad, msg in (("dave\tfather\t?", "unknown entity"), ("alice\tuncle\t?", "unknown relation"), ("?\tfather\tdave", "unknown entity"),
                     ("alice\tfather\tbob", "exactly one"), ("?\tfather\t?", "exactly one"), ("alice father ?", "three"),
                     ("alice\tfather", "three")):
        with pytest.raises(ValueError, match=msg):
            predict.parse_query(bad, 2, e2i, r2i)
    for bad, msg in (("x\t0\t?", "not an id"), ("1\t2\t?", "out of range"), ("1\t-1\t?", "out of range")):
        with pytest.raises(ValueError, match=msg):
            predict.parse_query(bad, 2)
    assert predict.relation_name(3, 2, {0: "father", 1: "mother"}) == "mother^-1"
    assert predict.relation_name(4, 2, {0: "father", 1: "mother"}) == "self"

