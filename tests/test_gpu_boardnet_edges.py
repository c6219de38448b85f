"""The board nets (nz_boardnet_*, nuzero_amd/csrc/boardnet.hip) at edge shapes against the FLOAT64 oracle
(oracle/net.py with dtype=float64), at the C ABI.  Cases, inputs, weights and the three error measures come from
tests/boardnet_cases.py; tests/test_boardnet_ref_host.py shows without a device that on these cases the float32 oracle
stays within 2e-6 of the float64 one, so the 1e-5 asserted here (BASELINE.json north_star, TOL of
tests/test_gpu_boardnet.py) allows the device 5x what the reference's own rounding costs, and that the cases are
neither flat nor saturated.

Every output buffer is a slice of a larger tensor with 64 sentinel floats before and after it, checked after every
call; every image batch is a slice with one sentinel position before and after it.

hex_odd: HexNetRef restates hexagdly's documented addressing; parity with hexagdly itself stays unpinned.

Needs a GPU."""
from ctypes import byref, c_int32, c_void_p

import numpy as np
import pytest

import boardnet_cases as bc

pytestmark = pytest.mark.gpu
TOL = bc.TOL
GUARD = 64
SENTINEL = -777.0
FORMS_TOL = 5e-6          # fused16_net_kernel against the per-layer kernels (tests/test_gpu_boardnet.py)
SURFACE_CASES = ["k1_odd", "rec_odd"]

_REF = {}


def _reference(case):
    """(inputs, float64 (logits, probs, value)) for the case's largest batch, computed once; smaller batches are its
    leading positions."""
    if case.name not in _REF:
        x = bc.inputs(case, max(max(bc.all_batches(case)), bc.SHARED_MAX_BATCH if case.name in SURFACE_CASES else 0))
        _REF[case.name] = (x, bc.reference64(case, x))
    return _REF[case.name]


def _want(case, lo, hi):
    x, (l, p, v) = _reference(case)
    return x[lo:hi], (l[lo:hi], p[lo:hi], v[lo:hi])


def _net(case, max_batch, w=None):
    from nuzero_amd.boardnet import BoardNet
    net = BoardNet(case.arch, case.in_channels, case.policy_channels, case.rows, case.cols, width=case.width,
                   num_blocks=case.depth, recall=case.recall, value_activation=case.value_activation,
                   kernel_size=case.kernel_size, max_batch=max_batch, hex=case.hex)
    net.set_weights(bc.weights(case) if w is None else w, case.iters)
    return net


class _Guarded:
    """A float32 device buffer of `count` floats between two guards of GUARD sentinel floats, itself pre-filled with
    the sentinel."""

    def __init__(self, count, shape):
        import torch
        self.whole = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.whole[GUARD:GUARD + count].view(shape)

    def ptr(self):
        return c_void_p(self.t.data_ptr())

    def guards_intact(self):
        return bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[-GUARD:] == SENTINEL).all())


def _images(x):
    """x on the device as a slice of a tensor with one sentinel position before and after it."""
    import torch
    whole = torch.full((len(x) + 2,) + x.shape[1:], 1.0e3, dtype=torch.float32, device="cuda")
    whole[1:-1].copy_(torch.from_numpy(x))
    return whole[1:-1]


def _outputs(net, n, logits=True, probs=True):
    A = net.num_actions
    return (_Guarded(n * A, (n, A)) if logits else None, _Guarded(n * A, (n, A)) if probs else None, _Guarded(n, (n,)))


def _forward(net, images, n, n_dev=None, logits=True, probs=True, stream=None, rows=False, outs=None):
    """nz_boardnet_forward (or _forward_rows) into guarded buffers -> (logits, probs, value) tensors (None where not
    requested), after checking the status and the guards."""
    import torch
    from nuzero_amd._lib import lib
    out_l, out_p, out_v = outs or _outputs(net, n, logits, probs)
    s = c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream)
    nd = c_void_p(n_dev.data_ptr()) if n_dev is not None else None
    if rows:
        st = lib.nz_boardnet_forward_rows(net._h, n, nd, out_l.ptr() if out_l else None, out_p.ptr() if out_p else None,
                                          out_v.ptr(), s)
    else:
        assert images.is_contiguous() and images.shape[0] == n
        st = lib.nz_boardnet_forward(net._h, c_void_p(images.data_ptr()), n, nd, out_l.ptr() if out_l else None,
                                     out_p.ptr() if out_p else None, out_v.ptr(), s)
    assert st == 0, (st, lib.nz_boardnet_last_error(net._h))
    torch.cuda.synchronize()
    for g in (out_l, out_p, out_v):
        assert g is None or g.guards_intact(), "a kernel wrote outside its output buffer"
    return (out_l.t if out_l else None), (out_p.t if out_p else None), out_v.t


def _held(tag, got, want):
    """The three measures and the probability sums within 1e-5 of the float64 reference."""
    l, p, v = (None if t is None else t.cpu().numpy() for t in got)
    assert all(np.isfinite(a).all() for a in (l, p, v) if a is not None), tag
    e = bc.errors(l, p, v, want)
    print(f"{tag}: " + " ".join(f"{k} {e[k]:.2e}" for k in sorted(e)))
    for k, err in e.items():
        assert err < TOL, (tag, k, err)
    if p is not None:
        assert np.max(np.abs(p.astype(np.float64).sum(axis=1) - 1.0)) < 1e-5, tag
    return e


def _forms(case, net, images, n, want, tag):
    """Run the one-launch form (where the handle has one) and the per-layer kernels; hold both to the reference and to
    each other: bit-equal for fused_net_kernel (RecurrentNets), within 5e-6 for fused16_net_kernel."""
    import torch
    results = {}
    if net.fused(True):
        results["one-launch"] = _forward(net, images, n)
        _held(f"{tag} one-launch", results["one-launch"], want)
    net.fused(False)
    results["per-layer"] = _forward(net, images, n)
    _held(f"{tag} per-layer", results["per-layer"], want)
    net.fused(True)
    if "one-launch" in results:
        (lf, pf, vf), (lu, pu, vu) = results["one-launch"], results["per-layer"]
        if case.arch == "recurrent":
            assert torch.equal(lf, lu) and torch.equal(pf, pu) and torch.equal(vf, vu), tag
        else:
            scale = lu.abs().amax(dim=1, keepdim=True) + 1.0
            assert float(((lf - lu).abs() / scale).max()) < FORMS_TOL and float((pf - pu).abs().max()) < FORMS_TOL, tag
            assert float((vf - vu).abs().max()) < FORMS_TOL, tag
    return results


STANDARD = [c.name for c in bc.CASES if c.batches]
BIG = [(c.name, n) for c in bc.CASES for n in c.big_batches]


@pytest.mark.parametrize("handle", ["own", "shared"])
@pytest.mark.parametrize("name", STANDARD)
def test_edge_shapes_equal_the_float64_oracle(name, handle):
    """n in {1, 15, 16, 17, 37}: on a handle with max_batch == n ("own"), and on ONE handle with max_batch = 300
    ("shared"), where a workgroup of the one-launch forms gets a different share of the positions."""
    case = bc.BY_NAME[name]
    shared = _net(case, bc.SHARED_MAX_BATCH) if handle == "shared" else None
    for n in case.batches:
        x, want = _want(case, 0, n)
        net = shared or _net(case, n)
        _forms(case, net, _images(x), n, want, f"{name} n={n} max_batch={net.max_batch}")
        if net is not shared:
            net.close()
    if shared:
        shared.close()


@pytest.mark.parametrize("name,n", BIG)
def test_large_batches_on_the_per_layer_kernels(name, n):
    """The batch sizes at which dispatch_conv picks conv_wide_kernel or an MT = 2 tile (and the n = 37 controls, where
    the same layers run on conv_kernel's MT = 1 tiles), one-launch form off."""
    case = bc.BY_NAME[name]
    x, want = _want(case, 0, n)
    net = _net(case, n)
    net.fused(False)
    _held(f"{name} n={n} per-layer", _forward(net, _images(x), n), want)
    net.close()


# ---- surfaces -----------------------------------------------------------------------------------------------------------
def _rows_layout(case, x, row_stride):
    """The input rows the header documents: row = ((position / 16) * hw + cell) * 16 + position % 16, channels
    contiguous up to row_stride, zeros in the padded channels and in the positions that fill up the last group."""
    n, c, hw = len(x), case.in_channels, case.rows * case.cols
    groups = (n + 15) // 16
    rows = np.zeros((groups, hw, 16, row_stride), np.float32)
    pos = np.arange(n)
    rows[pos // 16, :, pos % 16, :c] = x.reshape(n, c, hw).transpose(0, 2, 1)
    return rows.reshape(-1)


class _DevicePointer:
    """A raw device pointer as something torch.as_tensor can wrap without a copy."""

    def __init__(self, ptr, floats):
        self.__cuda_array_interface__ = {"shape": (floats,), "typestr": "<f4", "data": (ptr, False), "version": 2}


def _input_rows(net, floats):
    """The handle's own input rows (nz_boardnet_input_rows) as a flat torch tensor over the same memory, and the stride."""
    import torch
    from nuzero_amd._lib import lib
    ptr, stride = c_void_p(0), c_int32(0)
    assert lib.nz_boardnet_input_rows(net._h, byref(ptr), byref(stride)) == 0
    return torch.as_tensor(_DevicePointer(ptr.value, floats), device="cuda"), stride.value


def _equal(a, b):
    import torch
    return all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("route", ["one-launch", "per-layer"])
@pytest.mark.parametrize("name", SURFACE_CASES)
def test_forward_rows_equals_forward(name, route):
    """Rows filled by the caller in the header's layout give the same bits as nz_boardnet_forward on the same images;
    nz_boardnet_forward itself leaves exactly that layout in the buffer (zeros in the padded channels and in the
    positions that fill up the last group of 16); finite values in the padded channels change nothing (their weights
    are zero in every packed stream); and a smaller batch run over the rows a larger one left in place (positions past
    the live ones are stale, not zero) gives the live positions the same bits."""
    import torch
    case = bc.BY_NAME[name]
    x37, _ = _want(case, 0, 37)
    net = _net(case, 37)
    assert net.fused(route == "one-launch") or route == "per-layer"
    hw, groups = case.rows * case.cols, (37 + 15) // 16
    stride = (case.in_channels + 15) // 16 * 16
    rows, got_stride = _input_rows(net, groups * hw * 16 * stride)
    assert got_stride == stride
    want37 = _forward(net, _images(x37), 37)
    layout = _rows_layout(case, x37, stride)
    assert len(layout) == rows.numel()
    assert np.array_equal(rows.cpu().numpy(), layout)         # what nchw_to_rows_kernel left there
    fresh = _net(case, 37)
    fresh.fused(route == "one-launch")
    frows, _ = _input_rows(fresh, len(layout))
    frows.copy_(torch.from_numpy(layout))
    assert _equal(_forward(fresh, None, 37, rows=True), want37)
    # the padded channels meet zero weights: finite values there change nothing
    junk = layout.reshape(-1, stride).copy()
    junk[:, case.in_channels:] = 3.0
    frows.copy_(torch.from_numpy(junk.reshape(-1)))
    assert _equal(_forward(fresh, None, 37, rows=True), want37)
    # n = 17 over the 37 positions' rows: position 17 .. 31 of the second group keep their stale planes
    got17 = _forward(fresh, None, 17, rows=True)
    assert _equal(got17, [t[:17] for t in want37])
    _held(f"{name} rows n=17 {route}", got17, _want(case, 0, 17)[1])
    net.close(); fresh.close()


@pytest.mark.parametrize("name", SURFACE_CASES)
def test_handle_reused_from_a_large_batch_to_small_ones(name):
    """max_batch = 300: n = 300, then 1, then 17 (other positions than the large call's first ones).  Each small call is
    bit-equal to a handle's that never saw the large batch, on both routes, and is held to the reference."""
    case = bc.BY_NAME[name]
    net = _net(case, 300)
    x, want = _want(case, 0, 300)
    for route in ("one-launch", "per-layer"):
        assert net.fused(route == "one-launch") or route == "per-layer"
        _held(f"{name} n=300 {route}", _forward(net, _images(x), 300), want)
        for lo, n in ((100, 1), (50, 17)):
            xs, ws = _want(case, lo, lo + n)
            got = _forward(net, _images(xs), n)
            _held(f"{name} n={n} after 300 {route}", got, ws)
            fresh = _net(case, 300)
            fresh.fused(route == "one-launch")
            assert _equal(got, _forward(fresh, _images(xs), n)), (name, route, n)
            fresh.close()
    net.close()


@pytest.mark.parametrize("route", ["one-launch", "per-layer"])
@pytest.mark.parametrize("name", SURFACE_CASES)
def test_device_side_batch_count(name, route):
    """n_dev holding 0: status NZ_OK and every output buffer untouched.  n_dev holding m < n: rows below m are bit-equal
    to the full run, rows from m on keep their sentinels."""
    import torch
    case = bc.BY_NAME[name]
    n = 37
    x, want = _want(case, 0, n)
    net = _net(case, n)
    assert net.fused(route == "one-launch") or route == "per-layer"
    images = _images(x)
    full = _forward(net, images, n)
    _held(f"{name} n={n} {route}", full, want)
    for m in (0, 1, 16, 17):
        n_dev = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = _forward(net, images, n, n_dev=n_dev)
        for g, f in zip(got, full):
            assert torch.equal(g[:m], f[:m]), (name, route, m)
            assert bool((g[m:] == SENTINEL).all()), (name, route, m)
    net.close()


@pytest.mark.parametrize("name", SURFACE_CASES)
def test_set_weights_on_a_live_handle(name):
    """A second set of weights on a live handle gives a fresh handle's result with those weights (and the reference's);
    the first set again gives the first run's bits."""
    case = bc.BY_NAME[name]
    n = 37
    x, want = _want(case, 0, n)
    images = _images(x)
    w2 = bc.weights(case, seed=case.seed + 1000)
    net = _net(case, n)
    first = _forms(case, net, images, n, want, f"{name} first weights")
    net.set_weights(w2, case.iters)
    want2 = bc.reference64(case, x, w2)
    second = _forms(case, net, images, n, want2, f"{name} second weights")
    fresh = _net(case, n, w2)
    for route, got in second.items():
        assert fresh.fused(route == "one-launch") or route == "per-layer"
        assert _equal(got, _forward(fresh, images, n)), (name, route)
    fresh.close()
    net.set_weights(bc.weights(case), case.iters)
    for route, got in first.items():
        assert net.fused(route == "one-launch") or route == "per-layer"
        assert _equal(got, _forward(net, images, n)), (name, route)
    net.close()


@pytest.mark.parametrize("name", ["two_by_two", "rec_odd"])
def test_a_board_net_leaves_nothing_behind(name):
    """Twelve handles made, given weights, run in each form, given other weights, run and closed: the device's free
    memory after the twelfth is what it was after the second, give or take one handle (tests/test_gpu_scs_lifecycle.py,
    test_nothing_left_behind).  two_by_two holds both one-launch programs, rec_odd the float32 one and two-source
    layers."""
    import torch
    case = bc.BY_NAME[name]
    n = 17
    x, _ = _want(case, 0, n)
    images = _images(x)
    w1, w2 = bc.weights(case), bc.weights(case, seed=case.seed + 1000)

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        before = free()
        net = _net(case, bc.SHARED_MAX_BATCH, w1)
        assert net.fused(True)
        _forward(net, images, n)
        net.fused(False)
        _forward(net, images, n)
        net.fused(True)
        net.set_weights(w2, case.iters)
        _forward(net, images, n)
        held = before - free()
        net.close()
        return held

    readings, footprint = {}, 0
    for i in range(1, 13):
        held = cycle()
        if i in (2, 12):
            readings[i] = free()
        if i == 2:
            footprint = held                       # (cycle 1 also warms the tensor allocator up)
    print(f"{name}: free after cycle 2: {readings[2]}, after cycle 12: {readings[12]}, one handle holds {footprint} bytes")
    assert readings[12] >= readings[2] - footprint


@pytest.mark.parametrize("name", SURFACE_CASES)
def test_call_on_a_side_stream(name):
    """Images produced on a non-default stream and the network called on it with no synchronisation in between."""
    import torch
    case = bc.BY_NAME[name]
    n = 37
    x, want = _want(case, 0, n)
    net = _net(case, n)
    base = _images(x)
    expect = _forward(net, base, n)
    side = torch.cuda.Stream()
    outs = _outputs(net, n)                      # filled on the default stream ...
    torch.cuda.synchronize()                     # ... before anything is queued on `side`
    with torch.cuda.stream(side):
        whole = torch.full((n + 2,) + tuple(base.shape[1:]), 1.0e3, dtype=torch.float32, device="cuda")
        images = whole[1:-1]
        for k in range(8):                       # a chain of kernels the forward call has to queue behind
            images.copy_(base * float(k))
        images.copy_(base)
        got = _forward(net, images, n, stream=side, outs=outs)
        assert torch.equal(images, base)
    assert _equal(got, expect)
    _held(f"{name} side stream", got, want)
    net.close()


@pytest.mark.parametrize("name", SURFACE_CASES)
def test_optional_outputs(name):
    """probs_dev == NULL with logits requested, and the reverse: each filled output is bit-equal to the full call's."""
    import torch
    case = bc.BY_NAME[name]
    n = 17
    x, _ = _want(case, 0, n)
    net = _net(case, n)
    images = _images(x)
    for route in ("one-launch", "per-layer"):
        assert net.fused(route == "one-launch") or route == "per-layer"
        l, p, v = _forward(net, images, n)
        l1, p1, v1 = _forward(net, images, n, probs=False)
        assert p1 is None and torch.equal(l1, l) and torch.equal(v1, v), (name, route)
        l2, p2, v2 = _forward(net, images, n, logits=False)
        assert l2 is None and torch.equal(p2, p) and torch.equal(v2, v), (name, route)
        l3, p3, v3 = _forward(net, images, n, logits=False, probs=False)
        assert torch.equal(v3, v), (name, route)
    net.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _create(case, status, **over):
    from nuzero_amd import _lib
    from nuzero_amd._lib import lib
    d = dict(in_channels=case.in_channels, policy_channels=case.policy_channels, width=case.width, depth=case.depth,
             kernel_size=case.kernel_size, rows=case.rows, cols=case.cols, max_batch=16)
    d.update(over)
    desc = _lib.NetDesc(d["in_channels"], d["policy_channels"], d["width"], d["depth"], int(case.recall), _lib.NZ_ACT_TANH,
                        {"recurrent": _lib.NZ_ARCH_RECURRENT, "resnet": _lib.NZ_ARCH_RESNET,
                         "convnet": _lib.NZ_ARCH_CONVNET}[case.arch], d["kernel_size"], 0)
    h = c_void_p(0)
    st = lib.nz_boardnet_create(byref(h), byref(desc), d["rows"], d["cols"], d["max_batch"], 0)
    assert st == status, (over, st)
    if status != 0:
        assert not h.value and lib.nz_boardnet_last_error(None), over
    return h


def test_refusals_carry_a_status_and_a_message():
    """Each refusal returns the documented status and leaves a non-empty nz_boardnet_last_error.  (A head schedule that
    reaches 0 channels is not among them: weights.head_channels cannot produce one for a positive width --
    tests/test_boardnet_ref_host.py::test_head_schedule_never_reaches_zero_channels.)"""
    import torch
    from nuzero_amd import _lib
    from nuzero_amd._lib import lib
    from nuzero_amd.boardnet import BoardNet
    case = bc.BY_NAME["k1_odd"]
    for over in (dict(rows=0), dict(cols=0), dict(width=0), dict(max_batch=0), dict(kernel_size=2), dict(in_channels=0),
                 dict(policy_channels=0), dict(depth=-1)):
        _create(case, _lib.NZ_ERR_ARG, **over)
    lib.nz_boardnet_destroy(_create(case, _lib.NZ_OK))

    net = _net(case, 16)
    x, _ = _want(case, 0, 17)
    images = _images(x)
    value = _Guarded(17, (17,))
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    st = lib.nz_boardnet_forward(net._h, c_void_p(images.data_ptr()), 17, None, None, None, value.ptr(), stream)   # n > max_batch
    assert st == _lib.NZ_ERR_ARG and b"max_batch" in lib.nz_boardnet_last_error(net._h)
    st = lib.nz_boardnet_forward(net._h, c_void_p(images.data_ptr()), 16, None, None, None, None, stream)          # NULL value_dev
    assert st == _lib.NZ_ERR_ARG and b"value_dev" in lib.nz_boardnet_last_error(net._h)
    st = lib.nz_boardnet_forward(net._h, None, 16, None, None, None, value.ptr(), stream)                          # NULL images
    assert st == _lib.NZ_ERR_ARG and b"images_dev" in lib.nz_boardnet_last_error(net._h)
    torch.cuda.synchronize()
    assert bool((value.whole == SENTINEL).all())
    net.close()

    rec = bc.BY_NAME["rec_odd"]
    net = BoardNet(rec.arch, rec.in_channels, rec.policy_channels, rec.rows, rec.cols, width=rec.width,
                   num_blocks=rec.depth, recall=rec.recall, max_batch=16)
    with pytest.raises(_lib.NzError, match="recurrent_iterations") as err:
        net.set_weights(bc.weights(rec), 0)
    assert err.value.code == _lib.NZ_ERR_ARG
    with pytest.raises(_lib.NzError, match="no weights set"):       # and the handle stays unusable, not half set
        net.forward(torch.zeros((1, rec.in_channels, rec.rows, rec.cols), device="cuda"))
    net.close()

    # a live handle, one tensor too few: refused before anything is packed, and the old weights are gone with it
    net = _net(case, 17)
    want17 = _forward(net, images, 17)
    short = dict(list(bc.weights(case).items())[:-1])
    with pytest.raises(_lib.NzError, match="tensors") as err:
        net.set_weights(short, case.iters)
    assert err.value.code == _lib.NZ_ERR_ARG
    st = lib.nz_boardnet_forward(net._h, c_void_p(images.data_ptr()), 17, None, None, None, value.ptr(), stream)
    assert st == _lib.NZ_ERR_STATE and b"no weights set" in lib.nz_boardnet_last_error(net._h)
    net.set_weights(bc.weights(case), case.iters)              # the right weights: a fresh handle's bits
    assert _equal(_forward(net, images, 17), want17)
    net.close()

    # NULL handles: a status and a message in the handle-less slot
    dims = [c_int32(0) for _ in range(5)]
    avail = c_int32(0)
    ptr, stride = c_void_p(0), c_int32(0)
    for call in (lambda: lib.nz_boardnet_set_weights(None, None, 0, 1),
                 lambda: lib.nz_boardnet_fused(None, -1, byref(avail)),
                 lambda: lib.nz_boardnet_dims(None, *[byref(d) for d in dims]),
                 lambda: lib.nz_boardnet_input_rows(None, byref(ptr), byref(stride)),
                 lambda: lib.nz_boardnet_forward(None, c_void_p(images.data_ptr()), 1, None, None, None, value.ptr(), stream),
                 lambda: lib.nz_boardnet_forward_rows(None, 1, None, None, None, value.ptr(), stream)):
        _create(case, _lib.NZ_ERR_ARG, rows=0)                      # leaves "bad sizes" in the slot
        assert call() == _lib.NZ_ERR_ARG
        msg = lib.nz_boardnet_last_error(None)
        assert msg and b"null handle" in msg, msg
