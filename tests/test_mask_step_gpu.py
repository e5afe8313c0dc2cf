"""rg_mask_step called on its own (-m gpu) against tests/mask_ref.py: one step of learning an edge mask - the objective's chain rule,
the regularisers, Adam, the new gate and the per-(replica, row) sums - in fp64, under the project's stated tolerance through
tests/_util.assert_close_fp32: rtol 1e-4 / atol 2e-5 of the fp64 reference, or 4 x the fp32 restatement's own error.

Shapes: five rows of 0, 1, 63, 257 and RG_MASK_CHUNK + 1 edges (an empty first row; the last row is one edge longer than the kernel's
chunk, so its sum is two chunk sums), the same lengths reversed (an empty last row), R = 1 and 3 replicas, about a fifth of the edges
not free.  Inputs away from Adam's first-step sign sensitivity (mask_ref.make_inputs): step 1 from zero moments with both lambdas 0,
step 2 from step 1's moments with all lambdas.

Also: count_out is the count over the kernel's own gate_out, exactly; size_out is within (n + 8) * 2^-24 * sum g of the fp64 sum of
the kernel's own gate_out, n the row's free edges (n - 1 additions and the rounding of the terms' order, with room); an edge that is
not free keeps theta, m, v and gate_out bit for bit; two runs give equal bits; replica k is the n_rep = 1 call on its slices, bit for
bit; the argument errors.
The kernel's worst |got - ref64| / (atol + rtol |ref64|) over these cases, as measured on an MI355X: 0.013 for theta, 0.004 for m,
0.014 for v, 0.002 for gate, 0.001 for size - the fp32 numpy restatement's own: 0.017, 0.004, 0.014, 0.002, 0.001 - and size_out at
most 0.014 of its bound (information only, the assertions use the tolerance above).  Wall time of this file there: 3.0 s (5 tests)."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import mask_ref as MR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
LR = 0.05
CHUNK = 512
LENGTHS = {"empty_first": [0, 1, 63, 257, CHUNK + 1], "empty_last": [CHUNK + 1, 257, 63, 1, 0]}
FIELDS = ("theta", "m", "v", "gate", "size")


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _call(x, score, grad, lam_s, lam_e, state, t, rows=None):
    """engine.mask_step on the replicas ``rows`` of (score, grad, lambdas, state = dict(theta, m, v, gate) numpy): a dict of numpy
    arrays.  The state is copied to the device, so the caller's arrays stay as they are."""
    from red_gnn_amd import engine
    sl = slice(None) if rows is None else rows
    th, m, v, g = (_dev(state[k][sl]) for k in ("theta", "m", "v", "gate"))
    gate, size, count = engine.mask_step(_dev(x.offsets, torch.int64), _dev(x.free, torch.uint8), _dev(score[sl]), _dev(x.target),
                                         _dev(x.inv_scale), _dev(x.inv_n), _dev(lam_s[sl]), _dev(lam_e[sl]), _dev(grad[sl]), th, m, v, t,
                                         lr=LR, gate_out=g)
    torch.cuda.synchronize()
    assert gate is g
    return {k: a.cpu().numpy() for k, a in dict(theta=th, m=m, v=v, gate=gate, size=size, count=count).items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _check_step(tag, x, got, before, score, grad, lam_s, lam_e, t):
    ref = {dt: MR.step(x.offsets, x.free, score, x.target, x.inv_scale, x.inv_n, lam_s, lam_e, grad, before["theta"], before["m"],
                       before["v"], t, LR, dtype=dt, gate_in=before["gate"]) for dt in (np.float64, np.float32)}
    for name in FIELDS:
        r64, r32 = ref[np.float64][name], ref[np.float32][name]
        err = np.abs(got[name].astype(np.float64) - r64)
        print("%s %s: worst |got - ref64| / (atol + rtol |ref64|) %.3g (the fp32 restatement: %.3g)"
              % (tag, name, (err / (ATOL + RTOL * np.abs(r64))).max(initial=0), (np.abs(r32 - r64) / (ATOL + RTOL * np.abs(r64))).max(initial=0)))
        U.assert_close_fp32(got[name], r32, r64, RTOL, ATOL, "%s %s" % (tag, name))
    # ---- the statistics against the kernel's own gates
    free, row = x.free, x.row
    for k in range(got["gate"].shape[0]):
        g = got["gate"][k]
        own_count = np.bincount(row[free], weights=(g[free] > np.float32(0.5)), minlength=x.B)[:x.B].astype(np.int64)
        assert np.array_equal(got["count"][k], own_count), "%s: count_out of replica %d" % (tag, k)
        own = np.bincount(row[free], weights=g[free].astype(np.float64), minlength=x.B)[:x.B]
        bound = (x.n_free + 8) * 2.0 ** -24 * own
        err = np.abs(got["size"][k].astype(np.float64) - own)
        print("%s replica %d size_out: worst |got - fp64 sum of gate_out| / bound %.3g" % (tag, k, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), "%s: size_out of replica %d" % (tag, k)
    assert got["count"].dtype == np.int32 and (got["size"][:, x.n_free == 0] == 0).all() and (got["count"][:, x.n_free == 0] == 0).all()
    # ---- an edge that is not free keeps all four arrays, bit for bit
    for name in ("theta", "m", "v", "gate"):
        assert np.array_equal(_bits(got[name])[:, ~free], _bits(before[name])[:, ~free]), "%s: %s changed where the edge is not free" % (tag, name)
    assert not np.isnan(got["gate"][:, free]).any()


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("layout", list(LENGTHS))
def test_two_steps_against_the_reference(layout, R):
    x = MR.make_inputs(LENGTHS[layout], R, seed=7 + R)
    assert 0.1 < (~x.free).mean() < 0.3 and x.n_free.max() > CHUNK * 0.7
    sentinel = np.full((R, x.E), np.float32(-7.25))                           # gate_out where nothing is written: must stay
    before = dict(theta=x.theta, m=x.zeros, v=x.zeros, gate=sentinel)
    tag = "%s R=%d" % (layout, R)
    one = _call(x, x.score, x.grad, x.lambda0, x.lambda0, before, 1)
    _check_step(tag + " step 1", x, one, before, x.score, x.grad, x.lambda0, x.lambda0, 1)
    two = _call(x, x.score2, x.grad2, x.lambda_size2, x.lambda_ent2, one, 2)
    _check_step(tag + " step 2", x, two, one, x.score2, x.grad2, x.lambda_size2, x.lambda_ent2, 2)
    assert np.abs(two["theta"] - one["theta"])[:, x.free].min() > 0           # every free edge moved
    # ---- two runs: equal bits
    again = _call(x, x.score2, x.grad2, x.lambda_size2, x.lambda_ent2, one, 2)
    for name in FIELDS + ("count",):
        assert np.array_equal(_bits(again[name]), _bits(two[name])), "%s: two runs differ in %s" % (tag, name)
    # ---- replica k is the one-replica call on its slices
    for k in range(R):
        part = _call(x, x.score2, x.grad2, x.lambda_size2, x.lambda_ent2, one, 2, rows=slice(k, k + 1))
        for name in FIELDS + ("count",):
            assert np.array_equal(_bits(part[name]), _bits(two[name][k:k + 1])), "%s: replica %d differs from its own call in %s" % (tag, k, name)


def test_argument_errors_and_the_empty_call():
    from red_gnn_amd import _lib, engine
    L, p = _lib.lib(), _lib.ptr
    x = MR.make_inputs([3, 0, 9], 2, seed=1)
    R, E, B = 2, x.E, x.B
    f = lambda a: _dev(a)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    arrays = dict(offsets=_dev(x.offsets, torch.int64), free=_dev(x.free, torch.uint8), score=f(x.score), target=f(x.target),
                  inv_scale=f(x.inv_scale), inv_n=f(x.inv_n), lambda_size=f(x.lambda_size2), lambda_ent=f(x.lambda_ent2), grad=f(x.grad))
    state = dict(theta=f(x.theta), m=f(x.zeros), v=f(x.zeros), gate_out=nan(R, E), size_out=nan(R, B),
                 count_out=torch.full((R, B), -1, dtype=torch.int32, device="cuda"))
    keep = {k: v.clone() for k, v in state.items()}

    def raw(n_rep=R, batch=B, n_edges=E, step=1, null=None, beta1=0.9):
        a = {k: (None if k == null else p(v)) for k, v in {**arrays, **state}.items()}
        return L.rg_mask_step(n_rep, batch, n_edges, a["offsets"], a["free"], a["score"], a["target"], a["inv_scale"], a["inv_n"],
                              a["lambda_size"], a["lambda_ent"], a["grad"], LR, beta1, 0.999, 1e-8, step, a["theta"], a["m"], a["v"],
                              a["gate_out"], a["size_out"], a["count_out"], _lib.stream_ptr())

    for kw, text in ((dict(n_rep=0), b"n_rep"), (dict(n_rep=-2), b"n_rep"), (dict(step=0), b"step"), (dict(step=-1), b"step"),
                     (dict(n_rep=(1 << 31) // E + 1), b"overflows int32"), (dict(n_rep=(1 << 30), batch=B), b"overflows int32"),
                     (dict(beta1=1.0), b"beta1")) + tuple((dict(null=k), b"NULL argument") for k in {**arrays, **state}):
        assert raw(**kw) != 0 and text in L.rg_last_error(), kw
    assert raw(n_edges=0) == 0                                                # succeeds, launches nothing
    torch.cuda.synchronize()
    for k, v in state.items():                                                # nothing was enqueued by any of these
        assert torch.equal(v.view(torch.int32), keep[k].view(torch.int32)), k
    # ---- the wrapper's own checks
    args = [arrays[k] for k in ("offsets", "free", "score", "target", "inv_scale", "inv_n", "lambda_size", "lambda_ent", "grad")]
    th, m, v = state["theta"], state["m"], state["v"]
    for step in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="mask_step: step"):
            engine.mask_step(*args, th, m, v, step)
    with pytest.raises(ValueError, match="mask_step: free"):
        engine.mask_step(args[0], args[1][:-1], *args[2:], th, m, v, 1)
    with pytest.raises(ValueError, match="mask_step: score"):
        engine.mask_step(args[0], args[1], args[2][:1], *args[3:], th, m, v, 1)
    with pytest.raises(ValueError, match="mask_step: m "):
        engine.mask_step(*args, th, m.double(), v, 1)
    with pytest.raises(ValueError, match="mask_step: offsets"):
        engine.mask_step(args[0].int(), *args[1:], th, m, v, 1)
    gate, size, count = engine.mask_step(*args, th, m, v, 1, lr=LR)           # and it runs: gate_out None is a new array of zeros
    assert gate.shape == (R, E) and not gate[:, torch.as_tensor(~x.free).cuda()].any() and count.dtype == torch.int32
    assert engine.MASK_CHUNK == CHUNK
