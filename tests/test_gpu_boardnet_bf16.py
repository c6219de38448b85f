"""The board nets' opt-in plain-bf16 mode (nz_boardnet_precision(h, NZ_PREC_BF16), fused16_net_kernel<HEX, PREC_BF16>) on
the fused16 cases of tests/boardnet_cases.py, at the C ABI.

  1. the default is untouched: precision unset and precision set to float32 give equal bytes;
  2. layer by layer, immune to rounding flips: nz_boardnet_forward_dump hands out what every layer stored; each layer is
     recomputed in float64 from the device's OWN dumped inputs (exact bf16 values), and a stored value must be the bf16
     (round to nearest even) of some y within delta of that result, delta = the float32 accumulation's and the
     activation's error; at most 1 % of a layer's values may need the delta at all;
  3. the whole network: forward == forward_dump bit for bit, within E_case of the float64 emulation (the coarse bound
     tests/test_bf16_ref_host.py establishes), more than 1e-4 from the float32 mode, bit-exact across batch slots, batch
     sizes and handles, with the batch size in device memory, guard sentinels round every output;
  4. what the mode refuses, each with its message.
Needs a GPU."""
from ctypes import c_void_p

import numpy as np
import pytest

import bf16_net_ref as br
import boardnet_cases as bc
from test_gpu_boardnet_edges import SENTINEL, _Guarded, _forward, _images, _outputs

pytestmark = pytest.mark.gpu
BATCHES = bc.STANDARD_BATCHES               # 1, 15, 16, 17, 37
U32 = 2.0 ** -24                            # float32 unit roundoff
FLIP_CAP = 0.01                             # share of a layer's values that may differ from the RNE of the float64 result
_NETS = {}


def _net(case, max_batch, precision="bf16"):
    from nuzero_amd.boardnet import BoardNet
    net = BoardNet(case.arch, case.in_channels, case.policy_channels, case.rows, case.cols, width=case.width,
                   num_blocks=case.depth, recall=case.recall, value_activation=case.value_activation,
                   kernel_size=case.kernel_size, max_batch=max_batch, hex=case.hex, precision=precision)
    net.set_weights(bc.weights(case), case.iters)
    return net


def _shared(case, precision="bf16"):
    """The case's handle of SHARED_MAX_BATCH positions, made once per mode."""
    key = (case.name, precision)
    if key not in _NETS:
        _NETS[key] = _net(case, bc.SHARED_MAX_BATCH, precision)
    return _NETS[key]


def _x(case, n):
    return br.e_case(case.name)["x"][:n]     # (the first n positions of a draw are the draw of n)


def _forward_dump(net, images, n, n_dev=None):
    """nz_boardnet_forward_dump into guarded buffers -> (logits, probs, value, [sections as numpy])."""
    import torch
    from nuzero_amd._lib import lib
    layout = net.dump_layout()
    total = sum(n * r * c for r, c in layout)
    out_l, out_p, out_v = _outputs(net, n)
    dump = _Guarded(total, (total,))
    st = lib.nz_boardnet_forward_dump(net._h, c_void_p(images.data_ptr()), n, dump.ptr(), total,
                                      c_void_p(n_dev.data_ptr()) if n_dev is not None else None, out_l.ptr(), out_p.ptr(),
                                      out_v.ptr(), c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, (st, lib.nz_boardnet_last_error(net._h))
    torch.cuda.synchronize()
    for g in (out_l, out_p, out_v, dump):
        assert g.guards_intact(), "a kernel wrote outside its buffer"
    flat, at, sections = dump.t.cpu().numpy(), 0, []
    for r, c in layout:
        sections.append(flat[at:at + n * r * c].reshape(n, r, c))
        at += n * r * c
    return out_l.t, out_p.t, out_v.t, sections


def _planes(section, case, channels):
    """[n, rows, C] of a dump section (its hw position rows) -> float64 [n, channels, rows, cols]."""
    n, hw = section.shape[0], case.rows * case.cols
    return np.ascontiguousarray(section[:, :hw, :channels].astype(np.float64).transpose(0, 2, 1)).reshape(n, channels, case.rows,
                                                                                                  case.cols)


def _check_layers(case, sections, got, tag):
    """Test 2 for one forward_dump: every layer from the device's own dumped inputs."""
    hw = case.rows * case.cols
    ls = br.layers(case)
    wts = br.layer_weights(case, bc.weights(case))
    ntaps = 7 if case.hex else 9
    assert len(sections) == len(ls) + 1, tag
    # the rounded input: RNE of the planes, zero in the padded channels and in the row of zeros
    x = _x(case, sections[0].shape[0])
    assert np.array_equal(_planes(sections[0], case, case.in_channels), br.rne_bf16(x)), tag
    assert not sections[0][:, :hw, case.in_channels:].any() and not sections[0][:, hw, :].any(), tag
    cin = {0: case.in_channels}
    for L in ls:
        cin[L.index + 1] = L.cout
    rows32 = {}
    for L, wt in zip(ls, wts):
        sec = sections[L.index + 1]
        a = _planes(sections[L.src], case, cin[L.src])
        wr = tuple(br.rne_bf16(t) for t in wt)
        y = br.conv64(case, a, wr)
        s_abs = br.conv64(case, np.abs(a), tuple(np.abs(t) for t in wr))
        if L.res is not None:
            r = _planes(sections[L.res], case, cin[L.res])
            y, s_abs = y + r, s_abs + np.abs(r)
        products = ntaps * 32 * (((cin[L.src] + 15) // 16 * 16 + 31) // 32)   # every product of the chain, zero ones included
        delta = (products + 2) * U32 * s_abs
        want = br.activate(y, L.act)
        if L.act == 2:
            delta = delta + 2.0 ** -22 * np.abs(want)                           # tanhf; its slope is at most 1
        elif L.act == 3:
            delta = delta + 2e-7                                                # fast_expm1, slope at most 1
        stored = _planes(sec, case, L.cout)
        # channels from the layer's width to its last tile's end meet zero weights: exactly 0
        assert not sec[:, :hw, L.cout:].any(), (tag, L.index, "padded output channels")
        if L.rows32:
            assert sec.shape[1] == hw, tag
            rows32[L.index] = (stored, y)
            continue
        assert sec.shape[1] == hw + 1 and not sec[:, hw, :].any(), (tag, L.index, "the row of zeros")
        lo, hi = br.rne_bf16(want - delta), br.rne_bf16(want + delta)
        bad = (stored < lo) | (stored > hi)
        assert not bad.any(), (tag, L.index, int(bad.sum()), float(np.abs(stored - want)[bad].max()))
        flips = float(np.mean(stored != br.rne_bf16(want)))
        assert flips <= FLIP_CAP, (tag, L.index, flips)
    # the float32 rows, the softmax and the value: within 1e-5 of float64 on the dumped last inputs
    (pol_dev, pol64), (val_dev, val64) = (rows32[i] for i in sorted(rows32))
    want = br.outputs(case, pol64, val64)
    l, p, v = (t.cpu().numpy() for t in got)
    assert np.array_equal(pol_dev.reshape(len(l), -1).astype(np.float32), l), (tag, "the logits are the policy rows")
    e = bc.errors(l, p, v, want)
    print(f"{tag}: float32 tail " + " ".join(f"{k} {e[k]:.2e}" for k in sorted(e)))
    assert max(e.values()) < bc.TOL, (tag, e)
    assert max(bc.errors(None, None, np.tanh(val_dev.mean(axis=(1, 2, 3))), want).values()) < bc.TOL, tag


@pytest.mark.parametrize("name", ["k1_scs", "strip_col"])
def test_the_default_is_untouched(name):
    import torch
    from nuzero_amd.boardnet import BoardNet
    case = bc.BY_NAME[name]
    plain = BoardNet(case.arch, case.in_channels, case.policy_channels, case.rows, case.cols, width=case.width,
                     num_blocks=case.depth, value_activation=case.value_activation, kernel_size=case.kernel_size, max_batch=37,
                     hex=case.hex)
    plain.set_weights(bc.weights(case), case.iters)
    f32 = _net(case, 37, "float32")
    assert plain.precision == "float32" and f32.precision == "float32"
    for n in (1, 16, 37):
        im = _images(_x(case, n))
        a, b = _forward(plain, im, n), _forward(f32, im, n)
        for ta, tb in zip(a, b):
            assert torch.equal(ta.view(torch.int32), tb.view(torch.int32)), (name, n)
    plain.close(); f32.close()


@pytest.mark.parametrize("name", br.FUSED16_CASES)
def test_every_layer_from_the_device_s_own_inputs(name):
    case = bc.BY_NAME[name]
    for n in BATCHES:
        for net, label in ((_net(case, n), "own"), (_shared(case), "shared")):
            got = _forward_dump(net, _images(_x(case, n)), n)
            _check_layers(case, got[3], got[:3], f"{name} n={n} {label}")
            if label == "own":
                net.close()


@pytest.mark.parametrize("name", br.FUSED16_CASES)
def test_the_all_zero_position_gives_zero_outputs(name):
    import torch
    case = bc.BY_NAME[name]
    net = _shared(case)
    x = np.zeros((3, case.in_channels, case.rows, case.cols), np.float32)
    l, p, v, sections = _forward_dump(net, _images(x), 3)
    assert not l.any() and not v.any() and all(not s.any() for s in sections)
    assert float((p - 1.0 / net.num_actions).abs().max()) < 1e-7 / net.num_actions + 1e-9      # exp(0) / A


@pytest.mark.parametrize("name", br.FUSED16_CASES)
def test_the_whole_network(name):
    import torch
    case = bc.BY_NAME[name]
    e = br.e_case(name)
    net, ref32 = _shared(case), _shared(case, "float32")
    n = 37
    x = _x(case, n)
    im = _images(x)
    got = _forward(net, im, n)
    dumped = _forward_dump(net, im, n)
    for a, b in zip(got, dumped[:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, "forward is forward_dump")
    l, p, v = (t.cpu().numpy() for t in got)
    emu = tuple(a[:n] for a in e["emu"])
    d_emu = br.distance((l, p, v), emu)
    f32 = tuple(t.cpu().numpy().astype(np.float64) for t in _forward(ref32, im, n))
    d_f32 = br.distance((l, p, v), f32)
    print(f"{name}: to the float64 emulation {d_emu:.3e} (E_case {e['E']:.3e}), to the float32 mode {d_f32:.3e}")
    assert np.max(np.abs(p.astype(np.float64).sum(axis=1) - 1.0)) < 1e-5
    assert d_emu <= e["E"], (name, d_emu, e["E"])
    assert d_f32 > 1e-4, (name, d_f32, "is the mode on?")
    # the same position in other slots, batch sizes and handles: bit-exact
    own = _net(case, 17)
    order = np.array([5, 0, 16, 3, 3, 11, 36, 1, 20, 7, 9, 30, 2, 2, 8, 4, 35])
    for h, label in ((net, "shared"), (own, "max_batch 17")):
        lo, po, vo = _forward(h, _images(x[order]), len(order))
        idx = torch.from_numpy(order).cuda()
        assert torch.equal(lo.view(torch.int32), got[0][idx].view(torch.int32)), (name, label)
        assert torch.equal(po.view(torch.int32), got[1][idx].view(torch.int32)), (name, label)
        assert torch.equal(vo.view(torch.int32), got[2][idx].view(torch.int32)), (name, label)
    own.close()
    # the live batch size in device memory: 15 of the 37, nothing written past them
    n_dev = torch.tensor([15], dtype=torch.int32, device="cuda")
    outs = _outputs(net, n)
    ld, pd, vd = _forward(net, im, n, n_dev=n_dev, outs=outs)
    for a, b in zip((ld, pd, vd), got):
        assert torch.equal(a[:15].view(torch.int32), b[:15].view(torch.int32)), name
        assert bool((a[15:] == SENTINEL).all()), (name, "outputs past *n_dev")
    n_dev.zero_()
    outs = _outputs(net, n)
    for a in _forward(net, im, n, n_dev=n_dev, outs=outs):
        assert bool((a == SENTINEL).all()), (name, "*n_dev == 0 writes nothing")


def _error_of(fn):
    from nuzero_amd._lib import NzError
    with pytest.raises(NzError) as ei:
        fn()
    return ei.value


def test_what_the_mode_refuses():
    from nuzero_amd import _lib
    from nuzero_amd.boardnet import BoardNet
    rec = bc.BY_NAME["rec_odd"]
    net = BoardNet(rec.arch, rec.in_channels, rec.policy_channels, rec.rows, rec.cols, width=rec.width, num_blocks=rec.depth,
                   recall=rec.recall, max_batch=16, precision="bf16")
    err = _error_of(lambda: net.set_weights(bc.weights(rec), rec.iters))
    assert err.code == _lib.NZ_ERR_ARG and "RecurrentNet" in str(err)
    x = _images(bc.inputs(rec, 2))
    assert _error_of(lambda: net.forward(x)).code == _lib.NZ_ERR_STATE          # no float32 stand-in: no weights are set
    net.precision = "float32"                                                     # the same handle takes them in float32 mode
    net.set_weights(bc.weights(rec), rec.iters)
    net.forward(x)
    net.close()

    wide = bc.BY_NAME["nt3"]
    net = BoardNet(wide.arch, wide.in_channels, wide.policy_channels, wide.rows, wide.cols, width=wide.width,
                   num_blocks=wide.depth, kernel_size=wide.kernel_size, max_batch=16, precision="bf16")
    err = _error_of(lambda: net.set_weights(bc.weights(wide), 1))
    assert err.code == _lib.NZ_ERR_ARG and "wider than 64" in str(err)
    net.close()

    case = bc.BY_NAME["k1_scs"]
    net = _net(case, 16)
    err = _error_of(lambda: net.fused(False))
    assert err.code == _lib.NZ_ERR_STATE and "float32" in str(err)
    assert net.fused() is True
    net.forward(_images(_x(case, 4)))
    # a change of mode drops the weights; the dump exists in bf16 mode only
    net.precision = "float32"
    assert net.precision == "float32"
    err = _error_of(lambda: net.forward(_images(_x(case, 4))))
    assert err.code == _lib.NZ_ERR_STATE and "no weights" in str(err)
    net.set_weights(bc.weights(case), 1)
    err = _error_of(lambda: net.forward_dump(_images(_x(case, 4))))
    assert err.code == _lib.NZ_ERR_STATE and "bf16" in str(err)
    with pytest.raises(ValueError):
        net.precision = "fp8"
    assert _lib.lib.nz_boardnet_precision(net._h, 7, None) == _lib.NZ_ERR_ARG
    net.close()
