"""Attention profile, the parts that run without a GPU: the C-ABI's declaration, export and argument checks, the loud failure
without a device, the result type, the command line's parsing and table, and the numpy reference on a case computed by hand."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _util as U
from tests import profile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported():
    from red_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "redgnn.h")).read()
    assert re.search(r"\bint\s+rg_attn_profile\s*\(", header)
    assert "rg_attn_profile" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "rg_attn_profile"), "libredgnn.so does not export rg_attn_profile"       # (dlsym)
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT rg_attn_profile$", out, re.M), "rg_attn_profile is not a defined text symbol of libredgnn.so"


def test_attn_profile_reports_bad_arguments():
    """Non-zero status and a message before any device work (no frontier is ever dereferenced: it is NULL here)."""
    from red_gnn_amd import _lib
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = _lib.ptr(buf)
    names = ["f", "g", "batch", "n_ent", "level", "n_old", "a_s", "a_r", "a_q", "ap", "w_alpha", "b_alpha", "attn_dim", "sum_out",
             "count_out", "stream"]
    ok = dict(zip(names, (None, None, 2, 8, 1, 2, p, p, p, 4, p, p, 3, p, p, None)))

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return L.rg_attn_profile(*[a[n] for n in names])

    for kw, msg in ((dict(sum_out=None), b"NULL argument"), (dict(count_out=None), b"NULL argument"), (dict(a_s=None), b"NULL argument"),
                    (dict(a_r=None), b"NULL argument"), (dict(a_q=None), b"NULL argument"), (dict(w_alpha=None), b"NULL argument"),
                    (dict(b_alpha=None), b"NULL argument"),
                    (dict(level=0), b"level 0 not in"), (dict(level=16), b"level 16 not in"), (dict(level=-3), b"level -3 not in"),
                    (dict(attn_dim=33, ap=36), b"attn_dim=33"), (dict(attn_dim=0), b"attn_dim=0"), (dict(attn_dim=5, ap=4), b"attn_dim=5"),
                    (dict(ap=6, attn_dim=5), b"ap=6"),
                    (dict(batch=0), b"batch=0"), (dict(n_ent=-1), b"n_ent=-1"),
                    (dict(), b"NULL frontier or graph")):
        assert call(**kw) != 0, kw
        assert msg in L.rg_last_error(), (kw, L.rg_last_error())


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_attention_profile_fails_loudly_without_gpu():
    from red_gnn_amd import _lib
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    ids = U.load("tiny_fwd.npz")
    loader = DataLoader(ids=ids, verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = 2, 16, 3, loader.n_rel, "relu", 0.0

    model = RED_GNN_trans(P, loader)
    with pytest.raises(_lib.NativeError):
        model.attention_profile(ids["subs"], ids["rels"])
    with pytest.raises(_lib.NativeError):
        model.attention_profile(ids["subs"], ids["rels"], group="query")


def _hand_profile():
    """n_rel = 2 (5 relation rows: father, mother, father^-1, mother^-1, self), 2 hops, query relations 0 and 3."""
    from red_gnn_amd.profile import AttentionProfile
    count = torch.zeros((5, 2, 5), dtype=torch.int64)
    fixed = torch.zeros((5, 2, 5), dtype=torch.int64)
    one = 1 << 32
    count[0, 0, 4], fixed[0, 0, 4] = 2, one                 # mean 0.5
    count[0, 0, 1], fixed[0, 0, 1] = 4, 3 * one             # mean 0.75
    count[0, 1, 0], fixed[0, 1, 0] = 1, one // 4            # mean 0.25
    count[0, 1, 2], fixed[0, 1, 2] = 2, one // 2            # mean 0.25: tie, the smaller id first
    count[3, 1, 3], fixed[3, 1, 3] = 8, one                 # mean 0.125
    return AttentionProfile(fixed=fixed, count=count, group="relation")


def test_result_type_mean_top_and_sum():
    prof = _hand_profile()
    assert prof.axes == ("group", "hop", "relation") and prof.n_hops == 2
    assert prof.alpha_sum.dtype == torch.float64 and prof.alpha_sum[0, 0, 1].item() == 3.0
    m = prof.mean()
    assert m[0, 0, 1].item() == 0.75 and m[0, 0, 4].item() == 0.5 and m[3, 1, 3].item() == 0.125
    assert torch.isnan(m[1]).all() and torch.isnan(m[0, 0, 0])
    assert int(torch.isnan(m).sum()) == 50 - 5
    ids, mean = prof.top(0, k=3)
    assert ids.tolist() == [[1, 4, -1], [0, 2, -1]]
    assert mean[0, :2].tolist() == [0.75, 0.5] and mean[1, :2].tolist() == [0.25, 0.25] and torch.isnan(mean[:, 2]).all()
    ids, mean = prof.top(3, k=9)                             # k above the number of relation rows: clipped
    assert ids.shape == (2, 5) and ids[1].tolist() == [3, -1, -1, -1, -1] and (ids[0] == -1).all()
    for bad in (dict(row=5), dict(row=-1), dict(row=0, k=0), dict(row=0, k=True), dict(row=0, k=1.5)):
        with pytest.raises(ValueError):
            prof.top(**bad)
    two = prof + prof
    assert torch.equal(two.count, 2 * prof.count) and torch.equal(two.fixed, 2 * prof.fixed)
    tot = prof.total()
    assert tot.count.shape == (5, 1, 5) and tot.count[0, 0].tolist() == [1, 4, 2, 0, 2]
    from red_gnn_amd.profile import AttentionProfile
    with pytest.raises(ValueError):
        prof + AttentionProfile(prof.fixed, prof.count, group="query")
    from red_gnn_amd import profile
    assert profile.Q == 2.0 ** -33


def test_cli_arguments_and_table():
    import attn_profile as cli
    a = cli.parse_args(["--ids", "x.npz", "--checkpoint", "m.pt"])
    assert (a.split, a.k, a.out, a.batch, a.max_queries, a.data_path) == ("test", 5, None, 50, None, None)
    a = cli.parse_args(["--data_path", "d/", "--checkpoint", "m.pt", "--split", "valid", "-k", "2", "--out", "p.tsv"])
    assert (a.split, a.k, a.out, a.data_path, a.ids) == ("valid", 2, "p.tsv", "d/", None)
    for bad in (["--checkpoint", "m.pt"], ["--ids", "x.npz"], ["--ids", "x.npz", "--data_path", "d", "--checkpoint", "m.pt"],
                ["--ids", "x.npz", "--checkpoint", "m.pt", "--split", "train"], ["--ids", "x.npz", "--checkpoint", "m.pt", "-k", "0"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    prof = _hand_profile()
    lines = cli.format_profile(prof, 2, k=2, id2rel={0: "father", 1: "mother"})
    assert lines == [
        cli.HEADER,
        "father\t1\t1\tmother\t0.750000\t3.000000\t4",
        "father\t1\t2\tself\t0.500000\t1.000000\t2",
        "father\t2\t1\tfather\t0.250000\t0.250000\t1",
        "father\t2\t2\tfather^-1\t0.250000\t0.500000\t2",
        "mother^-1\t2\t1\tmother^-1\t0.125000\t1.000000\t8",
    ]
    assert all(len(ln.split("\t")) == 7 for ln in lines)
    ids_only = cli.format_profile(prof, 2, k=1)
    assert ids_only[1] == "0\t1\t1\t1\t0.750000\t3.000000\t4" and ids_only[-1] == "1^-1\t2\t1\t1^-1\t0.125000\t1.000000\t8"
    from red_gnn_amd.profile import AttentionProfile
    with pytest.raises(ValueError):
        cli.format_profile(AttentionProfile(prof.fixed, prof.count, group="query"), 2)


def test_profile_ref_on_five_edges_by_hand():
    """Two queries (relations 1 and 1), two hops, 3 relation rows.  Hop 1: (0, h, rel 2, t) alpha .5; (1, h, rel 0, t) alpha .25 twice
    (a duplicated fact counts twice).  Hop 2: (0, h, rel 2, t) alpha 1; (0, h, rel 1, t) alpha .125."""
    hop_edges = [np.array([[0, 4, 2, 4, 0, 0], [1, 3, 0, 5, 1, 1], [1, 3, 0, 5, 1, 1]]), np.array([[0, 4, 2, 4], [0, 4, 1, 7]])]
    hop_alpha = [np.array([0.5, 0.25, 0.25]), np.array([1.0, 0.125])]
    count, asum = R.profile_by_query(hop_edges, hop_alpha, 2, 3)
    exp_c = np.zeros((2, 2, 3), np.int64)
    exp_s = np.zeros((2, 2, 3))
    exp_c[0, 0, 2], exp_s[0, 0, 2] = 1, 0.5
    exp_c[1, 0, 0], exp_s[1, 0, 0] = 2, 0.5
    exp_c[0, 1, 2], exp_s[0, 1, 2] = 1, 1.0
    exp_c[0, 1, 1], exp_s[0, 1, 1] = 1, 0.125
    assert np.array_equal(count, exp_c) and np.array_equal(asum, exp_s)
    c, s = R.by_relation(count, asum, [1, 1], 3)
    assert c.shape == (3, 2, 3) and not c[0].any() and not c[2].any()
    assert np.array_equal(c[1], exp_c[0] + exp_c[1]) and np.array_equal(s[1], exp_s[0] + exp_s[1])
