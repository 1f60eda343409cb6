"""lcx_diag_batch (include/lcx_diag.h): many selections and moments in one pass, against the sequence of classic calls -- bit for bit,
the sign of zeros included -- and against tests/_diag_reference.py at that module's own bars, so that a misreading shared by the two
paths cannot pass.  The states are the crafted cases of tests/test_oracle_diagnostics.py: a workgroup's range of exactly CF_CAP
values and of CF_CAP + 1, a cell of 2100 between empty ones, cf_cells() at 64, 5 and 1, empty cells at group edges and at the
domain's end, 0-D, the knife edges of [lo, hi), multiplicity 0 in the order, dead storage slots.  Every refusal tested here is made
on the host; nothing hands the kernel a bad pointer."""
import copy
import ctypes as C

import numpy as np
import pytest

import _diag_reference as R
import _harness as h
import test_oracle_diagnostics as D
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

REALS = pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
NAMES = ["A1", "A2", "A1_api_default", "B_five", "B_big", "B_parcel", "C", "E"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def expressible(calls):
    return [c for c in calls if lgrngn.diag_batch_expressible(c)]


def built(name, real_t):
    """the object of D.run_case up to its first diagnostic"""
    case = D.CASES[name](real_t)
    th, rv, rhod, Cf = case.fields
    prt = h.hip_particles(case.oi, real_t)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **Cf)
    case.setup(prt)
    return case, prt


def kept(case, name):
    sub = expressible(case.calls)
    if name == "C":
        assert sub == case.calls                           # (case.expect is indexed by the position in the list)
    else:
        assert len(sub) >= 20, len(sub)
    return sub


def launches(prt):
    return prt.state_u64("raw_launches").astype(np.int64)


# ---------------------------------------------------------------------------------- 1: same bits as the call sequence, and right
@REALS
@pytest.mark.parametrize("name", NAMES)
def test_batch_gives_the_bits_of_the_call_sequence_and_they_are_right(name, real_t):
    case, prt = built(name, real_t)
    sub = kept(case, name)
    outs_b = prt.diag_batch(sub)                           # (the object's first diagnostic: nothing has read it in case E)
    assert outs_b.shape == (len(sub), prt.n_cell) and outs_b.dtype == real_t
    outs_c = D.collect(prt, sub)
    for i, (b, c) in enumerate(zip(outs_b, outs_c)):
        assert same_bits(b, c), ("request #%d %r" % (i, sub[i]), np.nonzero(bits(b) != bits(c))[0][:8])
    st = D.read_state(prt)
    if case.intended is not None:
        assert np.array_equal(st["ijk"], case.intended)
    oi = case.oi
    ref = R.DiagRef(st, (oi.nx, oi.ny, oi.nz), oi.dt, real_t)
    sub_case = copy.copy(case)
    sub_case.calls = sub
    D.check(ref, sub_case, list(outs_b), real_t)


# ---------------------------------------------------------------------------------- 2: an object nobody has read
@REALS
def test_batch_on_an_object_nobody_has_read(real_t):
    case, first = built("E", real_t)
    sub = kept(case, "E")
    outs_b = first.diag_batch(sub)
    raw = first.state_u64("raw_n").size
    assert raw > first.n_part, "the storage must still hold dead slots when the batch runs"
    _, second = built("E", real_t)
    outs_c = D.collect(second, sub)
    for i, (b, c) in enumerate(zip(outs_b, outs_c)):
        assert same_bits(b, c), "request #%d %r" % (i, sub[i])


# ---------------------------------------------------------------------------------- 3: after a production step, the ranking still owed
@REALS
def test_batch_after_a_production_step_pays_the_owed_ranking(real_t):
    oi = h.box_opts(4, 4, 4, 64, strict_fp=False, cond_solver=0, kernel=lgrngn.kernel_t.hall_pinsky_stratocumulus)
    th, rv, rhod, Cf = D.cast_fields(h.box_fields(oi), real_t)
    prt = h.hip_particles(oi, real_t)
    prt.init(th, rv, rhod, **Cf)
    opts = lgrngn.opts_t()
    for _ in range(2):
        prt.step_sync(opts, th, rv, rhod, **Cf)
        prt.step_async(opts)
    sub = expressible(D.standard_calls(real_t))
    outs_b = prt.diag_batch(sub)                           # (at once: nothing has read the order since the step)
    assert int(prt.state_u64("raw_coal_ranked")[0]) > 0, "the step's coalescence must have ranked for itself and left the order owed"
    outs_c = D.collect(prt, sub)
    for i, (b, c) in enumerate(zip(outs_b, outs_c)):
        assert same_bits(b, c), "request #%d %r" % (i, sub[i])
    assert (outs_b[0] > 0).all() and (outs_b[1:] != 0).any()


# ---------------------------------------------------------------------------------- 3b: a slab with neighbours answers for its own cells
def test_batch_on_the_slabs_of_a_decomposed_domain():
    """what a process of libcloudphxx_amd.multi holds: a single-device object with distmem boundaries (here two slabs in one process,
    h.LocalRing, migrants exchanged after a full step) -- each slab is served and gives the bits of its own classic calls"""
    real_t = np.float64
    oi = h.box_opts(6, 3, 4, 32)
    th, rv, rhod, Cf = h.box_fields(oi)
    ring = h.LocalRing(oi, 2, lambda o: h.hip_particles(o, real_t), h.dev_alloc)
    ring.init(th, rv, rhod, **Cf)
    ring.step(lgrngn.opts_t(), th, rv, rhod, **Cf)
    sub = expressible(D.standard_calls(real_t))
    for r, prt in enumerate(ring.prts):
        assert prt.n_cell == ring.nxl[r] * 3 * 4
        outs_b = prt.diag_batch(sub)
        outs_c = D.collect(prt, sub)
        for i, (b, c) in enumerate(zip(outs_b, outs_c)):
            assert same_bits(b, c), ("slab %d request #%d %r" % (r, i, sub[i]))
        assert (outs_b[0] > 0).all()


# ---------------------------------------------------------------------------------- 4: passes
@REALS
def test_passes_and_the_order_of_requests(real_t):
    case, prt = built("B_five", real_t)
    sub = kept(case, "B_five")
    rpp, scratch = prt.diag_batch_info()
    assert 1 <= rpp <= 32 and scratch == 2 * rpp * prt.n_cell * np.dtype(real_t).itemsize
    classic = D.collect(prt, sub)
    n_req = 2 * rpp + 1
    pick = [(7 * i + 3) % len(sub) for i in range(n_req)]  # (every entry several times, equal powers far apart in the list)
    assert set(pick) == set(range(len(sub)))
    l0 = launches(prt)
    outs = prt.diag_batch([sub[j] for j in pick])
    assert list(launches(prt) - l0) == [3, 1]              # (three passes of one launch each; the host waits once, at the end)
    for i, j in enumerate(pick):
        assert same_bits(outs[i], classic[j]), "request #%d = call %d %r" % (i, j, sub[j])
    perm = np.random.default_rng(5).permutation(n_req)
    outs_p = prt.diag_batch([sub[pick[p]] for p in perm])
    unperm = np.empty_like(outs_p)
    unperm[perm] = outs_p
    assert same_bits(unperm, outs)
    # launches and host waits of a pass do not depend on how many requests it holds, and are fewer than the classic calls' for two
    two = sub[1:3]
    l0 = launches(prt)
    prt.diag_batch(two)
    l1 = launches(prt)
    prt.diag_batch([sub[j % len(sub)] for j in range(rpp)])
    l2 = launches(prt)
    D.collect(prt, two)
    l3 = launches(prt)
    print("launches, waits: batch of 2", l1 - l0, "batch of", rpp, l2 - l1, "classic 2", l3 - l2)
    assert np.array_equal(l1 - l0, l2 - l1)
    assert ((l1 - l0) < (l3 - l2)).all()
    assert (l1 - l0)[1] == 1                               # (one host wait)


# ---------------------------------------------------------------------------------- 5: output forms
@REALS
def test_output_forms(real_t):
    import torch
    case, prt = built("A1", real_t)
    sub = kept(case, "A1")
    n_req, n_cell = len(sub), prt.n_cell
    want = prt.diag_batch(sub)
    host = np.full((n_req, n_cell), -7, dtype=real_t)
    assert prt.diag_batch(sub, out=host) is host and same_bits(host, want)
    t = torch.full((n_req, n_cell), -7, dtype=torch.float64 if real_t is np.float64 else torch.float32, device="cuda")
    torch.cuda.synchronize()
    prt.diag_batch(sub, out=lgrngn.DeviceArray(t.data_ptr(), (n_req, n_cell)))
    assert same_bits(t.cpu().numpy(), want)
    for device in (False, True):
        if device:
            tp = torch.full((n_req, n_cell + 7), -7, dtype=t.dtype, device="cuda")
            torch.cuda.synchronize()
            prt.diag_batch(sub, out=lgrngn.DeviceArray(tp.data_ptr(), (n_req, n_cell), (n_cell + 7, 1)))
            padded = tp.cpu().numpy()
        else:
            padded = np.full((n_req, n_cell + 7), -7, dtype=real_t)
            prt.diag_batch(sub, out=padded[:, :n_cell])
        assert same_bits(padded[:, :n_cell], want), device
        assert (padded[:, n_cell:] == -7).all(), device
    with pytest.raises(RuntimeError, match="unit stride"):
        prt.diag_batch(sub, out=np.zeros((n_cell, n_req), dtype=real_t).T)
    with pytest.raises(RuntimeError, match="dtype"):
        prt.diag_batch(sub, out=np.zeros((n_req, n_cell), dtype=np.float32 if real_t is np.float64 else np.float64))


# ---------------------------------------------------------------------------------- 6: classic state untouched
@REALS
def test_classic_state_untouched(real_t):
    case, prt = built("B_five", real_t)
    _, twin = built("B_five", real_t)
    sub = kept(case, "B_five")
    for p in (prt, twin):
        p.diag_wet_rng(1e-6, 1e-4)
        p.diag_wet_mom(3)
    before = prt.outbuf_array()
    assert same_bits(before, twin.outbuf_array()) and (before != 0).any()
    prt.diag_batch(sub)
    assert same_bits(prt.outbuf_array(), before)
    prt.diag_wet_mom(0)                                    # (no new selection: the one made before the batch is still there)
    twin.diag_wet_mom(0)
    got = prt.outbuf_array()
    assert same_bits(got, twin.outbuf_array())
    everything = prt.diag_batch([([("all",)], ("mom", "wet", 0))])[0]
    assert (got <= everything).all() and (got < everything).any() and (got != 0).any()


# ---------------------------------------------------------------------------------- 7: errors on a live object
def raises(text, f):
    with pytest.raises(RuntimeError) as e:
        f()
    assert text in str(e.value), str(e.value)


def test_errors_on_a_live_object(monkeypatch):
    real_t = np.float64
    case, prt = built("B_parcel", real_t)
    sub = kept(case, "B_parcel")
    arr, n_cell = lgrngn.diag_batch_requests(sub), prt.n_cell
    call = lambda req, n, out, stride, dev=0: prt._chk(prt._f("diag_batch")(prt._h, req, C.c_int(n), C.c_void_p(out), C.c_size_t(stride), C.c_int(dev)))
    out = np.full((len(sub), n_cell), -7, dtype=real_t)
    raises("libcloudph++: diag_batch: req_stride (0) < n_cell (1)", lambda: call(arr, len(sub), out.ctypes.data, 0))
    raises("libcloudph++: diag_batch: out == NULL with n_req > 0", lambda: call(arr, len(sub), None, n_cell))
    raises("libcloudph++: diag_batch: out == NULL with n_req > 0", lambda: call(arr, len(sub), None, n_cell, 1))
    raises("libcloudph++: diag_batch: n_req < 0", lambda: call(arr, -1, out.ctypes.data, n_cell))
    call(arr, 0, out.ctypes.data, n_cell)                  # n_req == 0: succeeds, writes nothing
    call(None, 0, None, 0)
    assert (out == -7).all()
    assert prt.diag_batch([]).shape == (0, n_cell)
    arr[2].count = 7
    raises("libcloudph++: diag_batch: request 2: unknown count 7", lambda: call(arr, len(sub), out.ctypes.data, n_cell))
    assert (out == -7).all()
    # a larger box for the stride check proper
    case, prt = built("B_five", real_t)
    out = np.full((2, prt.n_cell), -7, dtype=real_t)
    raises("req_stride (5) < n_cell (6)", lambda: prt._chk(prt._f("diag_batch")(prt._h, lgrngn.diag_batch_requests(sub[:2]), C.c_int(2), C.c_void_p(out.ctypes.data),
                                                                                 C.c_size_t(5), C.c_int(0))))
    assert (out == -7).all()
    # before init(): what diag_all does there -- an error with its text, or the answer of an object without super-droplets
    def outcome(f):
        try:
            return "ok", f()
        except RuntimeError as e:
            return "error", str(e)
    fresh_a, fresh_b = h.hip_particles(case.oi, real_t), h.hip_particles(case.oi, real_t)
    a = outcome(fresh_a.diag_all)
    b = outcome(lambda: fresh_b.diag_batch(sub[:2]))
    assert a[0] == b[0], (a, b)
    if a[0] == "error":
        assert a[1] == b[1], (a, b)
    else:
        assert b[1].shape == (2, 6) and (bits(b[1]) == 0).all()
    # the multi-device object
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    mul = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert mul.dev_count == 2
    raises("libcloudph++: diag_batch on a multi-device object is not built", lambda: mul.diag_batch(sub[:2]))
    raises("libcloudph++: diag_batch on a multi-device object is not built", mul.diag_batch_info)
