"""hn_conv_gemm_nt_stream (csrc/hn_gemm_stream.hip) held to exact references and to hn_conv_gemm_nt, bit for bit.

1. Exact integer cases (the method of test_gemm_exact_gpu.py): small-integer bf16 operands make every sum exact in fp32, so the bf16 output
   and both statistics arrays must equal the integer reference exactly, whatever the tile walk.  The shapes are the smallest that can go
   wrong: one row, one row short of / one row past a 64-row tile, two tiles, seven tiles and a ragged eighth; K of one to four 32-chunks
   with live channels short of KP; Nout with one, three and four live 16-cout groups in the second cout half; wg_limit 1 (one workgroup
   walks every tile), 3 (uneven shares), tiles + 2 (idle workgroups) and 0 (the device grid).
2. Random bf16 operands: output, psum and psq equal hn_conv_gemm_nt's on the same arguments bit for bit, for every activation code.
3. Refusals leave a sentinel-filled output untouched.
4. A captured launch replayed three times equals the eager launch."""
import itertools

import pytest
import torch

from tests.guards import SENT16, Guarded, dev
from tests.test_gemm_exact_gpu import _stats_check, _w_int, budget, exact, gen, ints, randn, seed_of

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
HN_ERR_UNSUPPORTED = 3


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


def cdiv(a, b):
    return (a + b - 1) // b


def stream_call(K, x, m, c0, wp, nout, kp, bias, act, out, ldc, psum, psq, wg_limit):
    K.lib().call("hn_conv_gemm_nt_stream", x.data_ptr(), x.stride(0), m, c0, K.ptr(wp), nout, kp, K.ptr(bias), act, out.ptr(), ldc,
                 psum.ptr() if psum is not None else None, psq.ptr() if psq is not None else None, wg_limit)


def tile_call(K, x, m, c0, wp, nout, kp, bias, act, out, ldc, psum, psq):
    K.lib().call("hn_conv_gemm_nt", x.data_ptr(), None, 0, 0, 0, 0, c0, 0, x.stride(0), 0, 0, m, K.ptr(wp), nout, kp, 1, K.ptr(bias), act,
                 out.ptr(), 0, ldc, 0, 0, psum.ptr() if psum is not None else None, psq.ptr() if psq is not None else None)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


ROWS = [1, 63, 64, 65, 127, 128, 64 * 7 + 5]
KSHAPES = [(8, 32), (40, 64), (112, 128), (128, 128)]
NOUTS = [72, 112, 128]


@pytest.mark.parametrize("nout", NOUTS)
@pytest.mark.parametrize("c0,kp", KSHAPES, ids=["c8k32", "c40k64", "c112k128", "c128k128"])
def test_stream_exact(K, c0, kp, nout):
    name = f"stream_c{c0}_k{kp}_n{nout}"
    g = gen(seed_of(name))
    assert K.kp32(c0) == kp
    w3 = _w_int(nout, c0, 1, g, density=0.3)
    wp = K.pack_conv_weight(w3.view(nout, c0, 1, 1).contiguous())[0]
    bias_t = torch.randint(-4, 5, (nout,), generator=g, device=dev()).float()
    ldc = nout + 24
    for m in ROWS:
        assert K.lib().query("hn_nt_stream_ok", m, c0, nout, kp) == 1
        assert K.lib().query("hn_nt_stat_tile", m, nout) == 64
        tiles = cdiv(m, 64)
        assert K.lib().query("hn_nt_stat_rows", m, nout) == tiles
        x = ints((m, c0), -2, 2, g, 0.3, width=c0 + 8)                  # ld0 = C0 + 8 > C0; the extra columns hold other integers
        xd = x.double()
        budget(float((xd.abs() @ w3[:, :, 0].abs().t().double()).max()) + 4, name)
        raw = xd @ w3[:, :, 0].t().double()
        for has_bias, act, stats in itertools.product((False, True), (0, 1), (False, True)):
            pre = raw + bias_t.double() if has_bias else raw
            want = (pre.clamp(min=0) if act == 1 else pre).to(BF16)
            for wg in (0, 1, 3, tiles + 2):
                tag = f"{name} M={m} bias={has_bias} act={act} stats={stats} wg_limit={wg}"
                out = Guarded(m, nout, ldc, BF16)
                psum = Guarded(tiles, nout) if stats else None
                psq = Guarded(tiles, nout) if stats else None
                stream_call(K, x, m, c0, wp, nout, kp, bias_t if has_bias else None, act, out, ldc, psum, psq, wg)
                torch.cuda.synchronize()
                exact(out.view, want, tag + " out", lambda ii: f"pixel tile {ii[0][0] // 64} of {tiles}")
                out.check(tag + " out")
                if stats:                                               # of bf16(conv + bias), BEFORE the activation
                    _stats_check(pre.to(BF16), psum.view, psq.view, 64, nout, tag)
                    psum.check(tag + " psum")
                    psq.check(tag + " psq")


@pytest.mark.parametrize("c0,nout", [(112, 112), (128, 72)], ids=["112to112", "128to72"])
def test_stream_equals_tile_kernel_bitwise(K, c0, nout):
    """random bf16 operands: the streaming launch and hn_conv_gemm_nt agree in every bit of the output and of both statistics arrays"""
    name = f"stream_eq_{c0}_{nout}"
    g = gen(seed_of(name))
    m, kp = 64 * 37 + 9, 128
    tiles = cdiv(m, 64)
    assert K.lib().query("hn_nt_stat_rows", m, nout) == tiles
    x = randn((m, c0), g, width=c0 + 8)
    wf = torch.randn((nout, c0, 1, 1), generator=g, device=dev()) * 0.1
    wp = K.pack_conv_weight(wf.contiguous())[0]
    bias_t = torch.randn((nout,), generator=g, device=dev())
    ldc = nout + 8
    for act, has_bias in ((0, False), (0, True), (1, True), (2, True), (3, True), (4, True)):
        b = bias_t if has_bias else None
        ref, rs, rq = Guarded(m, nout, ldc, BF16), Guarded(tiles, nout), Guarded(tiles, nout)
        tile_call(K, x, m, c0, wp, nout, kp, b, act, ref, ldc, rs, rq)
        for wg in (0, 3):
            tag = f"{name} act={act} bias={has_bias} wg_limit={wg}"
            out, ps, pq = Guarded(m, nout, ldc, BF16), Guarded(tiles, nout), Guarded(tiles, nout)
            stream_call(K, x, m, c0, wp, nout, kp, b, act, out, ldc, ps, pq, wg)
            torch.cuda.synchronize()
            for got, want, what in ((out, ref, "out"), (ps, rs, "psum"), (pq, rq, "psq")):
                nbad = int((bits(got.view) != bits(want.view)).sum())
                assert nbad == 0, f"{tag}: {nbad} {what} elements differ in bits from hn_conv_gemm_nt"
                got.check(f"{tag} {what}")


def test_stream_refusals_write_nothing(K):
    g = gen(seed_of("stream_refusals"))
    m = 130
    raw = K.lib().raw("hn_conv_gemm_nt_stream")
    st = torch.cuda.current_stream().cuda_stream

    def refused(what, c0, kp, nout, ldc, x_off=0, out_off=0):
        x = ints((m + 1, c0), -2, 2, g, width=c0 + 8)
        wp = torch.zeros((nout, kp), dtype=BF16, device=dev())
        out = Guarded(m + 1, nout, max(ldc, nout), BF16)
        rc = raw(x.data_ptr() + x_off, x.stride(0), m, c0, wp.data_ptr(), nout, kp, None, 0, out.ptr() + out_off, ldc, None, None, 0, st)
        torch.cuda.synchronize()
        assert rc == HN_ERR_UNSUPPORTED, (what, rc)
        assert bool((out.buf.view(torch.int16) == SENT16).all()), f"{what}: a refused call wrote to the output"

    assert K.lib().query("hn_nt_stream_ok", m, 160, 112, 160) == 0
    refused("KP 160", 160, 160, 112, 136)
    refused("Nout 64", 112, 128, 64, 88)
    refused("Nout 136", 112, 128, 136, 160)
    refused("ldc odd", 112, 128, 112, 113)
    refused("ldc % 8 != 0", 112, 128, 112, 116)
    refused("x misaligned", 112, 128, 112, 136, x_off=2)
    refused("out misaligned", 112, 128, 112, 136, out_off=2)
    # the same arguments in the domain are accepted (so the refusals above are the predicate's, not an argument slip)
    x = ints((m, 112), -2, 2, g, width=120)
    wp = torch.zeros((112, 128), dtype=BF16, device=dev())
    out = Guarded(m, 112, 136, BF16)
    assert raw(x.data_ptr(), x.stride(0), m, 112, wp.data_ptr(), 112, 128, None, 0, out.ptr(), 136, None, None, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((out.view == 0).all())
    out.check("accepted call")


def test_stream_graph_replay(K):
    """one launch captured in a graph and replayed three times equals the eager launch: the kernel carries no state"""
    g = gen(seed_of("stream_replay"))
    m, c0, nout, kp = 64 * 9 + 17, 112, 112, 128
    tiles = cdiv(m, 64)
    x = randn((m, c0), g, width=c0 + 8)
    wp = K.pack_conv_weight((torch.randn((nout, c0, 1, 1), generator=g, device=dev()) * 0.1).contiguous())[0]
    bias_t = torch.randn((nout,), generator=g, device=dev())
    ldc = nout + 8
    ref, rs, rq = Guarded(m, nout, ldc, BF16), Guarded(tiles, nout), Guarded(tiles, nout)
    stream_call(K, x, m, c0, wp, nout, kp, bias_t, 2, ref, ldc, rs, rq, 3)
    torch.cuda.synchronize()
    out, ps, pq = Guarded(m, nout, ldc, BF16), Guarded(tiles, nout), Guarded(tiles, nout)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream_call(K, x, m, c0, wp, nout, kp, bias_t, 2, out, ldc, ps, pq, 3)
    for rep in range(3):
        for t in (out, ps, pq):
            t.view.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in ((out, ref, "out"), (ps, rs, "psum"), (pq, rq, "psq")):
            assert bool((bits(got.view) == bits(want.view)).all()), f"replay {rep}: {what} differs from the eager launch"
            got.check(f"replay {rep} {what}")
