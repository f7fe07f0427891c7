"""Host-side checks of the joint-covariance / sampling ABI (no GPU): the five names in the header,
the ctypes table and the Julia shim, and gprx_batch_cov_bytes' arithmetic."""
import ctypes as C
import pathlib
import re

from gprx import _lib as L

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "gprx.h"
NAMES = ["gprx_batch_predict_cov", "gprx_batch_sample", "gprx_batch_cov_bytes", "gprx_gp_predict_cov", "gprx_gp_sample"]


def prototype_args(name):
    """Number of parameters of `name`'s prototype in gprx.h (comments stripped)."""
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_names_in_header_and_bindings():
    for n in NAMES:
        assert prototype_args(n) == len(L.SIGNATURES[n][1]), n
        assert hasattr(L.lib, n)
    assert L.lib.gprx_abi_version() == 3
    assert "#define GPRX_ABI_VERSION 3\n" in HEADER.read_text()


def test_julia_ccalls_follow_the_header():
    jl = (REPO / "gpr.jl_amd" / "julia" / "GPRx.jl").read_text()
    for n in ("gprx_gp_predict_cov", "gprx_gp_sample"):
        m = re.search(r"ccall\(\(:" + n + r", LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, n
        assert len([a for a in m.group(1).split(",") if a.strip()]) == prototype_args(n), n


def cov_bytes(B, N, M):
    out = C.c_uint64(0)
    rc = L.lib.gprx_batch_cov_bytes(B, N, M, C.byref(out))
    return rc, out.value


def pad(n):
    return max(64, (n + 63) // 64 * 64)


def test_cov_bytes_arithmetic():
    """8 B (Npad Mpad + 2 Mpad^2) for V^T, Sigma and its factor, plus the documented staging term
    8 B 2 Mpad^2 + 12 B (the Z and sample buffers, Mpad vectors per slot a pass; jitter, status)."""
    for B, N, M in [(1, 1, 0), (1, 1, 1), (3, 65, 7), (240, 2048, 100), (2, 130, 130), (5, 64, 1024)]:
        rc, v = cov_bytes(B, N, M)
        Np, Mp = pad(N), pad(M)
        assert rc == L.OK
        assert v == 8 * B * (Np * Mp + 2 * Mp * Mp) + 8 * B * 2 * Mp * Mp + 12 * B


def test_cov_bytes_exact_values():
    """gprx_batch_cov_bytes to the byte for (B, N, M_max), recorded from the library before the
    workspace's buffers were described in one list (tests/test_abi.py
    test_batch_bytes_exact_values: the same shapes, without d)."""
    recorded = {
        (1, 1, 0): 163852,
        (1, 64, 64): 163852,
        (2, 65, 129): 2752536,
        (3, 130, 16): 688164,
        (8, 2048, 100): 20971616,
        (3, 4096, 0): 6684708,
        (240, 2048, 100): 629148480,
        (1, 1000, 1025): 46792716,
    }
    for shape, want in recorded.items():
        assert cov_bytes(*shape) == (L.OK, want), shape


def test_cov_bytes_monotone():
    base = cov_bytes(4, 200, 100)[1]
    assert cov_bytes(5, 200, 100)[1] > base
    assert cov_bytes(4, 257, 100)[1] > base
    assert cov_bytes(4, 200, 129)[1] > base
    assert cov_bytes(4, 201, 101)[1] == base  # the same padded sizes


def test_cov_bytes_invalid_arguments():
    assert L.lib.gprx_batch_cov_bytes(1, 64, 64, None) == L.INVALID_ARGUMENT
    assert cov_bytes(0, 64, 64)[0] == L.INVALID_ARGUMENT
    assert cov_bytes(1, 0, 64)[0] == L.INVALID_ARGUMENT
    # N = 64, M = 20000: Npad Mpad 8 = 10 MB is addressable, Mpad^2 8 = 3.2 GB is not
    assert cov_bytes(1, 64, 20000) == (L.INVALID_ARGUMENT, 0)
    assert cov_bytes(1, 64, 16320)[0] == L.OK  # Mpad^2 8 = 2^31 - 17.8 MB: below the range
