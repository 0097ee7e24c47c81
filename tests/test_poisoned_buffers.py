"""Every kernel of the C ABI on poisoned buffers (tests/poison.py): guard bands around each operand, outputs
pre-filled with a NaN pattern no kernel writes, inputs framed by quiet NaNs, and the same launch repeated on
zero-filled buffers.  The rest of the suite compares results with the oracle or with earlier calls of the same
shape, whose outputs the caching allocator hands straight back -- so an unwritten row still holds the right
values there.  Here it cannot: skipped work, a store past the end, a read outside an operand and a read of a
workspace row before it is written all fail.

Also the dynamic work distribution of the persistent 16-bit kernel (kernel_mfma16.h, Sched16) against the
stream handles that do not name one ordered queue: hipStreamPerThread, more streams than pool slots, a stream
destroyed with work in flight and a new one created in its place."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import oracle
from hand_pose_sl_amd import _lib
from poison import POISON, Guarded, guarded_output, launch
from test_gpu_parity import ORACLE_MODE, TOL, TOL_MODEL
from test_transformer_enc import TOL as TENC_TOL
from test_transformer_enc import _load as tenc_load

pytestmark = pytest.mark.gpu

PIXELS = np.array([1280.0, 720.0], np.float32)
ALL_FLAGS = _lib.PRE_CHEST_DIFF | _lib.PRE_NORMALIZE | _lib.POST_DENORMALIZE | _lib.POST_MASK_TAIL
HIP_PER_THREAD = ctypes.c_void_p(2)  # hipStreamPerThread: one handle, a different stream in every host thread


def _conv(prec, C, dev, seed=0):
    torch.manual_seed(seed)
    m = hps.ConvModel(C, "ReLU", False, precision=prec).to(dev).eval()
    return m, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def _num_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _forward(m, prec, x, dev, stream=None):
    """b2h_forward of x (host or device, (B,T,12,2)) on poisoned buffers; returns y on the device."""
    lib = m._ensure_handle()
    B, T = x.shape[0], x.shape[1]

    def call(p):
        return lib.b2h_forward(m._handle, p["x"], p["y"], B, T, _lib.KERNELS[prec], stream)
    return launch(call, {"x": x}, {"y": (B, T, 21, 2)}, dev)["y"]


def _forward_fused(m, prec, body, nf, dev):
    lib = m._ensure_handle()
    B, T = body.shape[0], body.shape[1]

    def call(p):
        return lib.b2h_forward_fused(m._handle, p["x"], p["y"], B, T, ALL_FLAGS, 1280.0, p["nf"], _lib.KERNELS[prec], None)
    return launch(call, {"x": body, "nf": torch.as_tensor(nf, dtype=torch.int64)}, {"y": (B, T, 21, 2)}, dev)["y"]


def _vs_oracle(y, x, state, prec, rows=None):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    y = y.cpu().numpy()
    if rows is not None:
        x, y = x[rows], y[rows]
    ref = oracle.forward_from_state(x, state)
    err = np.abs(y - ref).max()
    assert err <= TOL[prec], (prec, err)
    if prec in ORACLE_MODE:
        errm = np.abs(y - oracle.forward_from_state(x, state, mode=ORACLE_MODE[prec])).max()
        assert errm <= TOL_MODEL[prec], (prec, errm)


def _fused_vs_oracle(y, body, nf, state, prec):
    inp, _ = oracle.preprocess(body, None)
    ref = oracle.postprocess(oracle.forward_from_state(inp, state), 1280.0, nf)
    y = y.cpu().numpy()
    assert np.abs(y - ref).max() <= 2 * TOL[prec] * 1280
    for b, n in enumerate(nf):
        assert not y[b, int(n):].any(), (prec, b, n)      # masked frames are written zeros


# ---- ConvModel: every kernel at the lengths where tiles and chunks end ------------------------------------------------
# (precision, conv_channels, what launch() runs for it)
CONV_MODELS = [("f32_valu", 30, "valu-c30"), ("f32_valu", 64, "valu-c57to104"), ("f32_valu", 96, "valu-c65to104"),
               ("f32_valu", 128, "valu-c105up-three-items"),
               ("f32_mfma", 30, "narrow"), ("f32_mfma", 48, "wide"), ("f16x3", 30, "narrow"), ("f16x3", 48, "wide"),
               ("bf16", 30, "persistent"), ("bf16", 48, "wide16"), ("f16", 30, "persistent"), ("f16", 48, "wide16")]
# tile / chunk edges: 16-frame tiles, T mod 32 in 13..16 (odd head tiles), 208 whole / 192 split 16-bit chunks,
# 112-frame fp32 chunks, 64-frame VALU tiles; 1000 = several chunks in every kernel
LENGTHS = [1, 15, 16, 17, 31, 32, 45, 48, 77, 208, 209, 400, 1000]


@pytest.mark.parametrize("prec,C,kind", CONV_MODELS, ids=[f"{p}-{k}" for p, _, k in CONV_MODELS])
def test_conv_lengths_on_poisoned_buffers(prec, C, kind, cuda_device):
    m, state = _conv(prec, C, cuda_device, seed=C)
    g = torch.Generator().manual_seed(C)
    for T in LENGTHS:
        x = torch.rand((3, T, 12, 2), generator=g) - 0.5
        _vs_oracle(_forward(m, prec, x, cuda_device), x, state, prec)
    rng = np.random.default_rng(C)
    for T in (17, 209):                                   # fused, tail mask at the edges and ragged
        body = rng.random((6, T, 12, 2), dtype=np.float32) * PIXELS
        nf = np.array([0, 1, T - 1, T, rng.integers(0, T + 1), rng.integers(0, T + 1)])
        _fused_vs_oracle(_forward_fused(m, prec, torch.from_numpy(body), nf, cuda_device), body, nf, state, prec)
    # B == 0: nothing is written, not even inside y
    lib = m._ensure_handle()
    x, y = Guarded(4 * 24, 0, 0, cuda_device), guarded_output(4 * 42, True, cuda_device)
    assert lib.b2h_forward(m._handle, x.ptr, y.ptr, 0, 1, _lib.KERNELS[prec], None) == _lib.OK
    torch.cuda.synchronize()
    assert y.guards_intact() and bool((y.body == POISON).all())


def _regimes():
    """(precision, conv_channels, B, T, id): every distribution launch() chooses, named.  B is a function of the
    CU count for the dynamic launch.  Chunk lengths at 256 CUs (launch(): 112-frame chunks unless fewer than
    2 chunks per wave slot, then 64, then 32; the one-wave-per-SIMD wide kernels have half the slots)."""
    out = []
    for prec in ("f32_mfma", "f16x3"):
        for C, bs, w in ((30, (3, 256, 1500), "narrow"), (48, (3, 128, 400), "wide")):
            out += [(prec, C, b, 300, f"{prec}-{w}-chunk{cl}") for b, cl in zip(bs, (32, 64, 112))]
    for prec in ("bf16", "f16"):
        out += [(prec, 30, 1500, 208, f"{prec}-whole208-static-stream"),
                (prec, 30, 1500, 400, f"{prec}-split192-static-stream"),
                (prec, 30, 400, 200, f"{prec}-chunk96"),
                (prec, 30, 2, 200, f"{prec}-chunk48"),
                (prec, 30, 2, 17, f"{prec}-static-below-stream-threshold"),
                (prec, 30, "dynamic", 16, f"{prec}-dynamic-stream"),
                (prec, 48, 400, 200, f"{prec}-wide16"),
                (prec, 48, 2, 17, f"{prec}-wide16-small")]
    return out


REGIMES = _regimes()


@pytest.mark.parametrize("prec,C,B,T", [r[:4] for r in REGIMES], ids=[r[4] for r in REGIMES])
def test_conv_dispatch_regimes_on_poisoned_buffers(prec, C, B, T, cuda_device):
    if B == "dynamic":
        B = 256 * _num_cus(cuda_device) + 37             # >= 256 chunks per workgroup: waves claim from the pool
    m, state = _conv(prec, C, cuda_device, seed=7)
    g = torch.Generator().manual_seed(B + T)
    x = (torch.rand((B, T, 12, 2), generator=g) - 0.5).to(cuda_device)
    y = _forward(m, prec, x, cuda_device)
    rows = sorted({0, 1, B // 2, B - 1})
    _vs_oracle(y, x, state, prec, rows)
    assert torch.equal(y[rows], _forward(m, prec, x[rows].contiguous(), cuda_device))  # any chunking, same bits
    rng = np.random.default_rng(B)
    body = (x + 0.5) * torch.from_numpy(PIXELS).to(cuda_device)
    nf = rng.integers(0, T + 1, size=B)
    nf[:min(B, 4)] = [0, 1, T - 1, T][:B]
    yf = _forward_fused(m, prec, body, nf, cuda_device)
    _fused_vs_oracle(yf[rows], body[rows].cpu().numpy(), nf[rows], state, prec)
    keep = torch.arange(T, device=cuda_device)[None, :] < torch.from_numpy(nf).to(cuda_device)[:, None]
    assert not yf[~keep].any()


# ---- TransformerEnc: output and workspace poisoned ------------------------------------------------------------------
def _tenc(dev, precision, max_len):
    state, cases = tenc_load()
    m = hps.TransformerEnc(24, 4, 128, 42, 4, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    m = m.to(dev).eval()
    if max_len != 100:
        m.pos_encoder = hps.PositionalEncoding(24, 0.5, max_len=max_len).to(dev)
        state = dict(state)
        state["pos_encoder.pe"] = m.pos_encoder.pe.cpu().numpy()
    return m, state, cases


def _tenc_forward(m, x, dev, ws=None, fused=None):
    lib = m._ensure_handle()
    assert lib.b2h_tenc_set_kernel(m._handle, hps.transformer_enc.TENC_KERNELS[m.precision]) == _lib.OK
    B, T = x.shape[0], x.shape[1]
    need = lib.b2h_tenc_workspace_bytes(m._handle, B, T)
    ws = ws if ws is not None else need
    nbytes = ws.nbytes if isinstance(ws, Guarded) else ws
    assert nbytes >= need
    inputs = {"x": x}
    if fused is not None:
        inputs["nf"] = torch.as_tensor(fused, dtype=torch.int64)

    def call(p):
        if fused is None:
            return lib.b2h_tenc_forward(m._handle, p["x"], p["y"], B, T, p["ws"], nbytes, None)
        return lib.b2h_tenc_forward_fused(m._handle, p["x"], p["y"], B, T, ALL_FLAGS, 1280.0, p["nf"], p["ws"], nbytes, None)
    return launch(call, inputs, {"y": (B, T, 21, 2)}, dev, scratch={"ws": ws})["y"]


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_tenc_on_poisoned_output_and_workspace(precision, cuda_device):
    m, state, cases = _tenc(cuda_device, precision, 100)
    for name, (x, y) in cases.items():                    # the reference's own vectors
        assert np.abs(_tenc_forward(m, torch.from_numpy(x), cuda_device).cpu().numpy() - y).max() <= TENC_TOL, name
    m, state, _ = _tenc(cuda_device, precision, 128)      # 101..128: the eight-tile attention
    g = torch.Generator().manual_seed(3)
    for T in (1, 17, 100, 128):
        for B in (3, 300):
            x = torch.rand((B, T, 12, 2), generator=g) - 0.5
            y = _tenc_forward(m, x, cuda_device).cpu().numpy()
            rows = sorted({0, B // 2, B - 1})
            ref = oracle.transformer_forward(x[rows].numpy(), state)
            assert np.abs(y[rows] - ref).max() <= TENC_TOL, (T, B)
    # fused transforms with a tail mask at the edges
    rng = np.random.default_rng(5)
    body = rng.random((5, 100, 12, 2), dtype=np.float32) * PIXELS
    nf = np.array([0, 1, 99, 100, 37])
    yf = _tenc_forward(m, torch.from_numpy(body), cuda_device, fused=nf).cpu().numpy()
    inp, _ = oracle.preprocess(body, None)
    ref = oracle.postprocess(oracle.transformer_forward(inp, state), 1280.0, nf)
    assert np.abs(yf - ref).max() <= 2 * TENC_TOL * 1280
    for b, n in enumerate(nf):
        assert not yf[b, n:].any()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_tenc_dirty_workspace_is_never_read_before_written(precision, cuda_device):
    """A workspace left dirty by a call of another shape (what the module's cached workspace holds) must give
    the same bits as a zero-filled one."""
    m, state, _ = _tenc(cuda_device, precision, 128)
    lib = m._ensure_handle()
    ws = Guarded(lib.b2h_tenc_workspace_bytes(m._handle, 40, 128), POISON, POISON, cuda_device)
    g = torch.Generator().manual_seed(9)
    x1 = torch.rand((40, 128, 12, 2), generator=g) - 0.5
    _tenc_forward(m, x1, cuda_device, ws=ws)              # poisoned workspace, then dirty with this call's rows
    for B, T in ((7, 33), (3, 128), (60, 17)):
        x = torch.rand((B, T, 12, 2), generator=g) - 0.5
        y = _tenc_forward(m, x, cuda_device, ws=ws).cpu().numpy()   # dirty workspace vs a zero-filled one
        assert np.abs(y - oracle.transformer_forward(x.numpy(), state)).max() <= TENC_TOL, (B, T)


# ---- metrics: per_seq and loss poisoned -------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["masked_l1", "weighted_l1"])
def test_metrics_on_poisoned_outputs(weighted, cuda_device):
    lib = _lib.load()
    g = torch.Generator().manual_seed(12)
    for B, T, lengths in ((5, 60, [60, 0, 33, 59, 1]), (257, 150, None), (300, 40, "ragged")):
        P, Tg, S = torch.rand((B, T, 21, 2), generator=g), torch.rand((B, T, 21, 2), generator=g), torch.rand((B, T, 21), generator=g)
        if lengths == "ragged":
            lengths = torch.randint(0, T + 1, (B,), generator=g).tolist()
            lengths[7] = 0
        inputs = {"p": P, "t": Tg, "s": S}
        if lengths is not None:
            inputs["nf"] = torch.tensor(lengths, dtype=torch.int64)

        def call(p):
            nf = p.get("nf")
            if weighted:
                return lib.b2h_weighted_l1(p["p"], p["t"], p["s"], nf, B, T, p["per"], p["loss"], None)
            return lib.b2h_masked_l1(p["p"], p["t"], nf, B, T, p["per"], p["loss"], None)
        out = launch(call, inputs, {"per": (B,), "loss": (1,)}, cuda_device)   # an empty sequence's NaN is computed
        per, loss = out["per"].cpu().numpy(), float(out["loss"].cpu()[0])
        if weighted:
            ref_loss, ref_per = oracle.weighted_l1(P.numpy(), Tg.numpy(), S.numpy(), lengths)
        else:
            ref_loss, ref_per = oracle.masked_l1(P.numpy(), Tg.numpy(), lengths)
        np.testing.assert_allclose(per, ref_per, rtol=5e-6)                    # NaN where the oracle has NaN
        if lengths is not None and 0 in list(lengths):
            assert np.isnan(loss) and np.isnan(ref_loss)
        else:
            assert abs(loss - float(ref_loss)) <= 2e-5 * max(1.0, abs(float(ref_loss)))


# ---- the dynamic claim counter and the stream handles it is keyed on --------------------------------------------------
def _dynamic_case(dev, prec="bf16", T=100, seed=0, model=None):
    """A fresh model (a corrupted pool slot cannot leak into other tests) and a batch with >= 256 chunks per
    workgroup, i.e. a DYNAMIC launch on a stream that owns a pool slot."""
    m, state = model if model is not None else _conv(prec, 30, dev, seed=seed)
    S = 256 * _num_cus(dev) + 37
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((S, T, 12, 2), generator=g) - 0.5).to(dev)
    return m, state, x


def _unwritten(buf):
    return int((buf.body == POISON).sum())


def _check_outputs(bufs, want, what):
    """Every guarded output equals `want` (flat int32 words); unwritten counts reported together."""
    torch.cuda.synchronize()
    report = [(i, b.guards_intact(), _unwritten(b), torch.equal(b.body, want)) for i, b in enumerate(bufs)]
    assert all(g and u == 0 and e for _, g, u, e in report), f"{what}: (launch, guards intact, unwritten words, equal) {report}"


def test_per_thread_default_stream_launches_from_two_threads(cuda_device):
    """hipStreamPerThread is the same handle in every host thread but a different stream in each: two threads
    doing dynamic launches on it must not share one claim counter (which would skip chunks and leave the
    finished-workgroup count of the slot non-zero for every later launch).  One thread runs 208-frame chunks,
    the other 16-frame ones: the persistent grids fill every CU, so a grid only starts as the other one drains,
    and it is the short chunks' early claims that meet the long chunks' tail."""
    prec = "bf16"
    m, _, x0 = _dynamic_case(cuda_device, prec, T=208, seed=1)
    _, _, x1 = _dynamic_case(cuda_device, prec, T=16, seed=4, model=(m, None))
    xs = [x0, x1]
    refs = [_forward(m, prec, xi, cuda_device).view(-1).view(torch.int32) for xi in xs]   # null stream, one at a time
    lib = m._ensure_handle()
    k = _lib.KERNELS[prec]
    outs = [[guarded_output(xi.shape[0] * xi.shape[1] * 42 * 4, True, cuda_device) for _ in range(3)] for xi in xs]
    torch.cuda.synchronize()
    start = threading.Barrier(2)
    rcs = [[], []]

    def worker(i):
        xi = xs[i]
        start.wait()
        for o in outs[i]:
            rcs[i].append(lib.b2h_forward(m._handle, ctypes.c_void_p(xi.data_ptr()), o.ptr, xi.shape[0], xi.shape[1], k,
                                          HIP_PER_THREAD))
        rcs[i].append(lib.b2h_stream_sync(HIP_PER_THREAD))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert rcs == [[0] * 4, [0] * 4], rcs
    for i in range(2):
        _check_outputs(outs[i], refs[i], f"thread {i}")
    for xi, ref in zip(xs, refs):                                   # the slots are clean afterwards
        again = guarded_output(xi.shape[0] * xi.shape[1] * 42 * 4, True, cuda_device)
        assert lib.b2h_forward(m._handle, ctypes.c_void_p(xi.data_ptr()), again.ptr, xi.shape[0], xi.shape[1], k, None) == 0
        _check_outputs([again], ref, "single-stream launch after the threads")


def _hip():
    """The HIP runtime torch loaded (libamdhip64.so.7, which libb2h also binds to: one runtime)."""
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    for fn in ("hipStreamDestroy", "hipStreamSynchronize", "hipStreamQuery"):
        getattr(hip, fn).argtypes = [ctypes.c_void_p]
    return hip


def test_more_streams_than_pool_slots(cuda_device):
    """70 distinct streams on one model: the first ones get a pool slot each (64 per model), the rest run the
    STATIC distribution -- every output complete and identical."""
    prec = "f16"
    m, _, x = _dynamic_case(cuda_device, prec, T=16, seed=2)
    B, T = x.shape[0], x.shape[1]
    ref = _forward(m, prec, x, cuda_device).view(-1).view(torch.int32)
    hip = _hip()
    lib = m._ensure_handle()
    streams = []
    try:
        for _ in range(70):
            s = ctypes.c_void_p()
            assert hip.hipStreamCreate(ctypes.byref(s)) == 0
            streams.append(s)
        assert len({s.value for s in streams}) == 70
        outs = [guarded_output(B * T * 42 * 4, True, cuda_device) for _ in streams]
        torch.cuda.synchronize()
        for s, o in zip(streams, outs):
            assert lib.b2h_forward(m._handle, ctypes.c_void_p(x.data_ptr()), o.ptr, B, T, _lib.KERNELS[prec], s) == _lib.OK
        for s in streams:
            assert hip.hipStreamSynchronize(s) == 0
        _check_outputs(outs, ref, "70 streams")
    finally:
        torch.cuda.synchronize()
        for s in streams:
            hip.hipStreamDestroy(s)


def test_destroyed_stream_handle_reused_by_a_new_stream(cuda_device):
    """Dynamic work on stream A, hipStreamDestroy(A) while it still runs, a new stream B (which can get A's handle
    value, and with it A's pool slot), dynamic work on B: all outputs complete and right, and a further launch on
    B too.  A runs 208-frame chunks and B 16-frame ones, so B's claims would meet A's tail if the destroy did not
    wait for A (see the per-thread test)."""
    import time
    prec = "bf16"
    m, _, xa = _dynamic_case(cuda_device, prec, T=208, seed=3)
    _, _, xb = _dynamic_case(cuda_device, prec, T=16, seed=5, model=(m, None))
    refs = [_forward(m, prec, xi, cuda_device).view(-1).view(torch.int32) for xi in (xa, xb)]
    hip = _hip()
    lib = m._ensure_handle()
    k = _lib.KERNELS[prec]

    def out(xi):
        return guarded_output(xi.shape[0] * xi.shape[1] * 42 * 4, True, cuda_device)

    def fwd(xi, o, s):
        return lib.b2h_forward(m._handle, ctypes.c_void_p(xi.data_ptr()), o.ptr, xi.shape[0], xi.shape[1], k, s)
    oa, ob = [out(xa) for _ in range(2)], [out(xb) for _ in range(2)]
    torch.cuda.synchronize()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(a)) == 0
    for o in oa:
        assert fwd(xa, o, a) == _lib.OK
    busy = hip.hipStreamQuery(a) == 600                    # hipErrorNotReady: A still had work when destroyed
    a_value = a.value
    t0 = time.perf_counter()
    assert hip.hipStreamDestroy(a) == 0
    destroy_ms = (time.perf_counter() - t0) * 1e3
    assert hip.hipStreamCreate(ctypes.byref(b)) == 0
    try:
        print(f"stream A busy at destroy: {busy}; hipStreamDestroy took {destroy_ms:.2f} ms; "
              f"B reuses A's handle: {b.value == a_value}")
        assert fwd(xb, ob[0], b) == _lib.OK
        assert hip.hipStreamSynchronize(b) == 0
        _check_outputs(oa, refs[0], "A (destroyed)")
        _check_outputs(ob[:1], refs[1], "B")
        assert fwd(xb, ob[1], b) == _lib.OK
        assert hip.hipStreamSynchronize(b) == 0
        _check_outputs(ob[1:], refs[1], "B again")
    finally:
        torch.cuda.synchronize()
        hip.hipStreamDestroy(b)
