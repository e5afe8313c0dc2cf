"""rg_mask_tie_grad and rg_mask_tie_gates called on their own (-m gpu) against tests/mask_tie_ref.py.

rg_mask_tie_grad's sum is defined (include/redgnn.h: chunks of RG_MASK_TIE_CHUNK = 32 members counted from the group's own first
member, a chunk added in member order from its first value, the chunk sums in chunk order), so the condition is on BITS: the kernel
equals the np.float32 loop of mask_tie_ref.group_sums32 on random floats, and on small-integer gradients, which are exact in any
order.  Next to it the project's stated tolerance, rtol 1e-4 / atol 2e-5 of the fp64 sums, asserted directly.

Shapes: groups of 0, 1, 2, 31, 32, 33, 64, 65 and 1025 members (empty, one member, one chunk less one, exactly one chunk, one more -
the first cut group -, two chunks, two and one, 33 chunks) and the same sizes reversed; the members are a shuffled subset of 1501
edges, so 248 edges are in no group; R = 1 and 3 replicas.  Also: replica k of the R = 3 call has the bits of an R = 1 call on its
slice; two calls give equal bits; a member out of range reads the clamped cell; rg_mask_tie_gates copies the group's bits to the
tied cells and stores nothing elsewhere (a sentinel stays), with about a fifth of the edges untied in runs that straddle the
kernel's four-edge accesses and an odd E, so that replica rows are only dword-aligned; every argument error and the empty calls
through raw _lib calls.
As measured on an MI355X: the bits are the reference's in every case; the worst |got - ref64| on the random floats is 2.8e-6, 0.0098
of the stated tolerance (information only).  Wall time of this file there: 2.6 s (8 tests)."""
import numpy as np
import pytest
import torch

from tests import mask_tie_ref as TR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
CHUNK = 32
E = 1501
SIZES = {"ascending": [0, 1, 2, 31, 32, 33, 64, 65, 1025], "descending": [1025, 65, 64, 33, 32, 31, 2, 1, 0]}


def _dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _layout(name, seed=3):
    sizes = np.array(SIZES[name], np.int64)
    rng = np.random.default_rng(seed)
    member = rng.permutation(E)[:sizes.sum()].astype(np.int32)                # a shuffled subset: no order, no edge twice
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert sizes.sum() == 1253 and len(np.unique(member)) == 1253
    return ptr, member


def _grad(R, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "floats":
        return rng.uniform(-1, 1, (R, E)).astype(np.float32)
    return rng.integers(-8, 9, (R, E)).astype(np.float32)                     # |sum| <= 8 * 1025: exact in float32 in any order


def _call(ptr, member, grad, host=True):
    from red_gnn_amd import engine
    out = engine.mask_tie_grad(_dev(ptr, torch.int32), _dev(member, torch.int32), _dev(grad, torch.float32), len(ptr) - 1,
                               grp_ptr_host=ptr if host else None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("layout", list(SIZES))
def test_grad_is_the_defined_sum_bit_for_bit(layout, R):
    ptr, member = _layout(layout)
    for kind in ("floats", "integers"):
        grad = _grad(R, kind, seed=11 + R)
        got = _call(ptr, member, grad)
        want32, want64 = TR.group_sums32(ptr, member, grad, CHUNK), TR.group_sums64(ptr, member, grad)
        tag = "%s R=%d %s" % (layout, R, kind)
        err = np.abs(got.astype(np.float64) - want64)
        print("%s: worst |got - ref64| %.3g, / (atol + rtol |ref64|) %.3g" % (tag, err.max(), (err / (ATOL + RTOL * np.abs(want64))).max()))
        assert got.dtype == np.float32 and got.shape == (R, len(ptr) - 1)
        assert np.array_equal(_bits(got), _bits(want32)), tag + ": not the defined sum"
        assert (err <= ATOL + RTOL * np.abs(want64)).all(), tag + ": beyond the stated tolerance of the fp64 sums"
        if kind == "integers":
            assert np.array_equal(got.astype(np.float64), want64), tag
        empty = np.diff(ptr) == 0
        assert empty.sum() == 1 and not _bits(got[:, empty]).any(), tag + ": an empty group is +0"
        # ---- two calls: equal bits; without the host pointer (the wrapper copies it back): equal bits
        assert np.array_equal(_bits(_call(ptr, member, grad)), _bits(got)), tag + ": two runs differ"
        assert np.array_equal(_bits(_call(ptr, member, grad, host=False)), _bits(got)), tag
        # ---- replica k is the one-replica call on its slice
        for k in range(R if R > 1 else 0):
            assert np.array_equal(_bits(_call(ptr, member, grad[k:k + 1])), _bits(got[k:k + 1])), "%s: replica %d differs from its own call" % (tag, k)
    # the cut matters: the sums of the cut groups are not those of one run over all members (or the test would not see a wrong cut)
    grad = _grad(1, "floats", seed=12)
    assert not np.array_equal(_bits(TR.group_sums32(ptr, member, grad, CHUNK)), _bits(TR.group_sums32(ptr, member, grad, 1 << 20)))


def test_one_member_keeps_its_bits_and_a_bad_member_reads_the_clamped_cell():
    ptr = np.array([0, 1, 2, 3, 5, 5, 40], np.int32)
    member = np.array([3, 0, E + 100, -5, 2] + list(range(10, 45)), np.int32)  # (in a call of its own: the wrapper does not check members)
    grad = _grad(2, "floats", seed=4)
    grad[:, 3], grad[0, 0] = -0.0, np.float32(1e-42)                          # -0 and a subnormal: a one-member group hands on the bits
    got = _call(ptr, member, grad)
    fixed = np.clip(member, 0, E - 1)
    assert np.array_equal(_bits(got), _bits(TR.group_sums32(ptr, fixed, grad, CHUNK)))
    assert np.array_equal(_bits(got[:, 0]), _bits(grad[:, 3])) and np.array_equal(_bits(got[:, 1]), _bits(grad[:, 0]))
    assert np.array_equal(_bits(got[:, 2]), _bits(grad[:, E - 1])) and np.array_equal(got[:, 3], grad[:, 0] + grad[:, 2])


@pytest.mark.parametrize("R", [1, 3])
def test_gates_copy_the_groups_bits_and_store_nothing_else(R):
    from red_gnn_amd import engine
    rng = np.random.default_rng(9 + R)
    G = 37
    group_of = rng.integers(0, G, E).astype(np.int32)
    # about a fifth untied, in runs of 1 .. 7 edges starting anywhere: inside one four-edge access, across two, covering whole ones
    while (group_of < 0).mean() < 0.2:
        a = rng.integers(0, E)
        group_of[a:a + rng.integers(1, 8)] = -1
    group_of[E - 1], group_of[E - 2], group_of[0] = -1, 5, -1                 # the array's last, partial four; the first cell
    untied = group_of < 0
    quads = untied[:E - E % 4].reshape(-1, 4).sum(1)
    assert 0.2 <= untied.mean() < 0.3 and {0, 1, 2, 3, 4} <= set(quads.tolist()) and E % 4 == 1
    grp_gate = rng.uniform(0, 1, (R, G)).astype(np.float32)
    sentinel = np.float32(-7.25)
    out = torch.full((R, E), float(sentinel), device="cuda")
    back = engine.mask_tie_gates(_dev(group_of, torch.int32), _dev(grp_gate, torch.float32), out)
    torch.cuda.synchronize()
    assert back is out
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:, ~untied]), _bits(grp_gate[:, group_of[~untied]])), "a tied cell is not its group's gate"
    assert (got[:, untied] == sentinel).all(), "a cell that is not tied was written"
    # a group beyond the array is clamped to the last one
    far = np.where(untied, -1, G + 5).astype(np.int32)
    out2 = torch.full((R, E), float(sentinel), device="cuda")
    engine.mask_tie_gates(_dev(far, torch.int32), _dev(grp_gate, torch.float32), out2)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out2.cpu().numpy()[:, ~untied]), _bits(np.repeat(grp_gate[:, -1:], (~untied).sum(), 1)))
    for k in range(R if R > 1 else 0):                                        # replica k is its own call
        one = torch.full((1, E), float(sentinel), device="cuda")
        engine.mask_tie_gates(_dev(group_of, torch.int32), _dev(grp_gate[k:k + 1], torch.float32), one)
        assert torch.equal(one[0], out[k])


def test_argument_errors_and_the_empty_calls():
    from red_gnn_amd import _lib, engine
    L, p = _lib.lib(), _lib.ptr
    ptr_h = np.array([0, 3, 3, 40, 41], np.int32)                             # one cut group: the call needs scratch
    G, M, R, n_e = 4, 41, 2, 64
    member = _dev(np.arange(M) % n_e, torch.int32)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    arrays = dict(grp_ptr=_dev(ptr_h, torch.int32), member=member, grad=torch.ones((R, n_e), device="cuda"), grp_grad=nan(R, G))
    need = int(L.rg_mask_tie_grad_scratch_bytes(p(ptr_h), G, R))
    assert need > 0 and int(L.rg_mask_tie_grad_scratch_bytes(p(np.array([0, 3, 3, 35, 36], np.int32)), G, R)) == 0
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def raw(n_rep=R, n_edges=n_e, n_groups=G, n_member=M, host=ptr_h, null=None, nbytes=need, buf=scratch):
        a = {k: (None if k == null else p(v)) for k, v in arrays.items()}
        return L.rg_mask_tie_grad(n_rep, n_edges, n_groups, n_member, a["grp_ptr"], None if null == "grp_ptr_host" else p(host), a["member"],
                                  a["grad"], a["grp_grad"], p(buf), nbytes, _lib.stream_ptr())

    bad = lambda *v: np.array(v, np.int32)
    for kw, text in ((dict(n_rep=0), b"n_rep"), (dict(n_rep=-2), b"n_rep"), (dict(n_edges=-1), b"negative size"),
                     (dict(n_groups=-1), b"negative size"), (dict(n_member=-1), b"negative size"),
                     (dict(n_rep=(1 << 31) // n_e + 1), b"overflows int32"), (dict(n_rep=(1 << 31) // G + 1, n_edges=1), b"overflows int32"),
                     (dict(n_rep=(1 << 31) // 5 + 1, n_edges=1), b"overflows int32"),       # the 4 groups and the 2 chunks of the cut one: 6 items a replica
                     (dict(host=bad(1, 3, 3, 40, 41)), b"starts at 1"), (dict(host=bad(0, 3, 2, 40, 41)), b"decreases at group 1"),
                     (dict(host=bad(0, 3, 3, 40, 40)), b"ends at 40"), (dict(n_member=M + 1), b"ends at 41"),
                     (dict(n_edges=0), b"no edge"), (dict(nbytes=need - 1), b"scratch"), (dict(buf=None), b"scratch")) \
            + tuple((dict(null=k), b"NULL argument") for k in list(arrays) + ["grp_ptr_host"]):
        assert raw(**kw) != 0 and text in L.rg_last_error(), (kw, L.rg_last_error())
    assert raw(n_groups=0, n_member=0, host=bad(0)) == 0                      # succeeds, launches nothing
    torch.cuda.synchronize()
    assert bool(torch.isnan(arrays["grp_grad"]).all())                        # nothing was enqueued by any of these
    assert raw() == 0                                                         # ... and the call itself runs
    torch.cuda.synchronize()
    assert arrays["grp_grad"].tolist() == [[3.0, 0.0, 37.0, 1.0]] * R
    # ---- rg_mask_tie_gates
    group_of, grp_gate, gate_out = _dev(np.arange(n_e) % G, torch.int32), torch.ones((R, G), device="cuda"), nan(R, n_e)

    def raw_gates(n_rep=R, n_edges=n_e, n_groups=G, null=None):
        a = {k: (None if k == null else p(v)) for k, v in dict(group_of=group_of, grp_gate=grp_gate, gate_out=gate_out).items()}
        return L.rg_mask_tie_gates(n_rep, n_edges, n_groups, a["group_of"], a["grp_gate"], a["gate_out"], _lib.stream_ptr())

    for kw, text in ((dict(n_rep=0), b"n_rep"), (dict(n_edges=-1), b"negative size"), (dict(n_groups=-3), b"negative size"),
                     (dict(n_rep=(1 << 31) // n_e + 1), b"overflows int32"), (dict(n_rep=(1 << 31) // G + 1, n_edges=1), b"overflows int32"),
                     (dict(null="group_of"), b"NULL argument"), (dict(null="grp_gate"), b"NULL argument"), (dict(null="gate_out"), b"NULL argument")):
        assert raw_gates(**kw) != 0 and text in L.rg_last_error(), kw
    assert raw_gates(n_edges=0) == 0 and raw_gates(n_groups=0) == 0           # succeed, launch nothing
    torch.cuda.synchronize()
    assert bool(torch.isnan(gate_out).all())
    # ---- the wrappers' own checks, and their empty calls
    gp, gr = arrays["grp_ptr"], arrays["grad"]
    for args, text in (((gp, member, gr, -1), "n_groups"), ((gp, member, gr, True), "n_groups"), ((gp, member, gr.double(), G), "grad"),
                       ((gp, member, gr[0], G), "grad"), ((gp.long(), member, gr, G), "grp_ptr"), ((gp[:-1], member, gr, G), "grp_ptr"),
                       ((gp, member.long(), gr, G), "member"), ((gp, member[:-1], gr, G), "grp_ptr must start at 0")):
        with pytest.raises(ValueError, match="mask_tie_grad: " + text):
            engine.mask_tie_grad(*args)
    assert engine.mask_tie_grad(gp[:1], member[:0], gr, 0).shape == (R, 0)
    assert engine.mask_tie_grad(torch.zeros(4, dtype=torch.int32, device="cuda"), member[:0], gr, 3).tolist() == [[0.0] * 3] * R
    for args, text in (((group_of, grp_gate, gate_out.double()), "gate_out"), ((group_of.long(), grp_gate, gate_out), "group_of"),
                       ((group_of[:-1], grp_gate, gate_out), "group_of"), ((group_of, grp_gate[:1], gate_out), "grp_gate"),
                       ((group_of, grp_gate.double(), gate_out), "grp_gate")):
        with pytest.raises(ValueError, match="mask_tie_gates: " + text):
            engine.mask_tie_gates(*args)
    assert engine.mask_tie_gates(group_of, grp_gate[:, :0].contiguous(), gate_out) is gate_out and bool(torch.isnan(gate_out).all())
    assert engine.MASK_TIE_CHUNK == CHUNK
