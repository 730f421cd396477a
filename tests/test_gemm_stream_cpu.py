"""CPU: the domain of hn_conv_gemm_nt_stream as the library states it (hn_nt_stream_ok) equals the Python-side predicate that routes
k_gemm_nt launches (ops.nt_stream_ok), over a grid that includes the model's shapes and both sides of every bound; the new source is part
of the library's build."""
import itertools

import pytest


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


def test_stream_source_is_built():
    from multitask_hydranet_amd import _lib
    assert "hn_gemm_stream.hip" in _lib.SOURCES
    assert any(s.endswith("hn_gemm_stream.hip") for s in _lib.sources())


def test_stream_predicate_matches_library(K):
    rows = [0, 1, 63, 64, 2048, 8192, 8193, 32768, 65536, 131072, 174592, 262144, 262145, 1 << 21]      # P7 ... P3, towers, both tile thresholds
    c0s = [0, 4, 8, 40, 64, 88, 112, 120, 128, 136, 160]
    nouts = [56, 64, 68, 72, 88, 112, 120, 128, 132, 136, 256]
    kps = [0, 16, 32, 64, 96, 128, 160]
    n_true = 0
    for m, c0, nout, kp in itertools.product(rows, c0s, nouts, kps):
        want = K.nt_stream_ok(m, c0, nout, kp)
        assert bool(K.lib().query("hn_nt_stream_ok", m, c0, nout, kp)) == want, (m, c0, nout, kp)
        if want:                                                      # inside the domain the statistics rows are those of the 64-row tiling
            assert K.lib().query("hn_nt_stat_tile", m, nout) == 64 and K.lib().query("hn_nt_stat_rows", m, nout) == (m + 63) // 64
            n_true += 1
    assert n_true > 100
    for m in (174592, 131072, 32768):                                 # det towers, BiFPN P3 / P4: 112 -> 112
        assert K.nt_stream_ok(m, 112, 112, 128)
    assert K.NT_STREAM_MAX_ROWS == 262144 and 0 < K.NT_STREAM_MIN_ROWS <= K.NT_STREAM_MAX_ROWS


def test_stream_null_pointers_are_rejected_without_a_gpu(K):
    raw = K.lib().raw("hn_conv_gemm_nt_stream")
    assert raw(None, 120, 4096, 112, None, 112, 128, None, 0, None, 112, None, None, 0, None) == 1
