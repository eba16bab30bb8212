"""CPU tier: the C-ABI library builds for gfx950, loads, and exports every
symbol that include/nmsa.h declares (no compute calls without a GPU)."""
import ctypes

import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L


def test_library_builds_and_exports_declared_symbols():
    path = L.build()
    handle = ctypes.CDLL(path)
    declared = L.declared_symbols()
    assert len(declared) >= 10
    for name in declared:
        assert hasattr(handle, name), f'{name} declared in nmsa.h but not exported'
    # every declared symbol has a ctypes signature in the binding (and vice versa)
    assert sorted(L._SIGNATURES.keys()) == declared


def test_targets_route_is_a_host_only_query():
    """`nmsa_targets_route` looks at its pointers for NULL and alignment only (the addresses here
    point nowhere) and answers without a device: the NMSA_TG_ROUTE_* mask the dispatchers of the
    target generators switch on, or NMSA_ERR_ARG for what they refuse"""
    lib = L.lib()
    assert 'nmsa_targets_route' in L.declared_symbols()
    U8, I16, I32, I64 = L.NMSA_U8, L.NMSA_I16, L.NMSA_I32, L.NMSA_I64
    SCAN, FAST, TILED, VECTOR, LUT, S16 = (
        L.NMSA_TG_ROUTE_SCAN, L.NMSA_TG_ROUTE_FAST_LOADERS, L.NMSA_TG_ROUTE_PAINT_TILED,
        L.NMSA_TG_ROUTE_PAINT_VECTOR, L.NMSA_TG_ROUTE_LUT_LDS, L.NMSA_TG_ROUTE_SCAN_16)
    assert (SCAN, FAST, TILED, VECTOR, LUT, S16) == (1, 2, 4, 8, 16, 32)
    base = 1 << 20

    def route(sem=base, sd=U8, ins=2 * base, idt=I32, NC=19, H=64, W=248, sigma=2, mi=1024,
              center=None, offset=None, fg=None, cm=None, ws=None):
        return lib.nmsa_targets_route(sem, sd, ins, idt, NC, H, W, sigma, mi, center, offset, fg, cm, ws)

    assert route() == SCAN | FAST | TILED | LUT
    assert route(mi=1025) == route(mi=4096) == SCAN | FAST | TILED | LUT | S16
    assert route(W=250) == FAST | VECTOR | LUT                   # H*W % 4 == 0, W % 4 != 0
    assert route(H=63, W=251) == LUT
    assert route(sigma=14) & LUT and not route(sigma=15) & LUT and not route(sigma=64) & LUT
    for shift in (1, 2, 3):
        assert route(sem=base + shift) == LUT
    for shift in (4, 8, 12):
        assert route(ins=2 * base + shift) == LUT
    for sd in (U8, I16, I32, I64):
        for idt in (U8, I16, I32, I64):
            assert bool(route(sd=sd, idt=idt) & SCAN) == ((sd, idt) == (U8, I32))
            if (sd, idt) != (U8, I32):
                assert route(sd=sd, idt=idt) == LUT
    assert route(NC=16384) & SCAN and route(NC=16385) == FAST | TILED | LUT
    assert route(ws=base + 8) == FAST | TILED | LUT              # the scan wants 16-byte aligned tables
    assert route(center=base + 4) == SCAN | FAST | LUT           # the paint falls back on its own
    assert route(W=250, offset=base + 8) == FAST | LUT
    assert route(fg=base + 2) == SCAN | FAST | LUT and route(cm=base + 1) == SCAN | FAST | LUT
    ERR_ARG = -1
    assert route(sem=None) == ERR_ARG and route(ins=None) == ERR_ARG
    assert route(sd=-1) == ERR_ARG and route(sd=4) == ERR_ARG and route(idt=4) == ERR_ARG
    assert route(NC=0) == ERR_ARG and route(NC=65537) == ERR_ARG
    assert route(H=0) == ERR_ARG and route(W=0) == ERR_ARG and route(H=32768) == ERR_ARG
    assert route(sigma=0) == ERR_ARG and route(sigma=65) == ERR_ARG
    assert route(mi=0) == ERR_ARG and route(mi=4097) == ERR_ARG
    assert route(ws=base + 4) == ERR_ARG                         # the generators want 8-byte alignment


def test_gauss_lut_has_one_entry_per_squared_distance():
    """`ops._gauss_lut`: 2 (3 sigma + 1)^2 + 1 float32 entries, float32(exp(-d2 / (2 sigma^2)));
    sigma = 14 is the last one the paint kernels keep in LDS (4096 entries)"""
    import numpy as np
    from nicr_mt_scene_analysis_amd import ops
    for sigma in (1, 8, 14, 15, 20, 64):
        lut = ops._gauss_lut(sigma, torch.device('cpu'))
        n = 2 * (3 * sigma + 1) ** 2 + 1
        assert lut.dtype == torch.float32 and tuple(lut.shape) == (n,)
        assert (n <= 4096) == (sigma <= 14)
        want = np.exp(-np.arange(n, dtype=np.float64) / (2 * sigma ** 2)).astype(np.float32)
        assert lut.numpy().tobytes() == want.tobytes()
        assert lut[0] == 1.0 and (lut[1:] < lut[:-1]).all() and lut[-1] > 0
    assert ops._gauss_lut(64, torch.device('cpu')).numel() == 74499


def test_version_and_error_strings():
    lib = L.lib()
    assert lib.nmsa_version() >= 100
    assert lib.nmsa_strerror(0) == b'ok'
    assert b'argument' in lib.nmsa_strerror(-1)


def test_device_geometry_query_and_override(monkeypatch):
    """grids are sized from what the HIP runtime reports for the device (csrc/api.hip); without a
    device the MI355X's numbers; NMSA_ASSUME_CUS / NMSA_ASSUME_XCDS override per call — and the
    workspace of the cooperating-workgroup cosine kernel follows (fewer CUs: fewer groups)"""
    monkeypatch.delenv('NMSA_ASSUME_CUS', raising=False)
    monkeypatch.delenv('NMSA_ASSUME_XCDS', raising=False)
    cus, xcds, lds = L.device_geometry()
    assert cus >= 1 and 1 <= xcds <= cus and lds >= 64 * 1024
    if not torch.cuda.is_available():
        assert (cus, xcds, lds) == (256, 8, 160 * 1024)
    full = L.lib().nmsa_loss_cos_emb_fwd_grad_workspace_bytes(2, 768, 256, 512, 64)
    monkeypatch.setenv('NMSA_ASSUME_CUS', '64')
    monkeypatch.setenv('NMSA_ASSUME_XCDS', '2')
    assert L.device_geometry()[:2] == (64, 2)
    quarter = L.lib().nmsa_loss_cos_emb_fwd_grad_workspace_bytes(2, 768, 256, 512, 64)
    assert 0 < quarter < full
    monkeypatch.setenv('NMSA_ASSUME_XCDS', '4096')             # never more XCDs than CUs
    assert L.device_geometry()[:2] == (64, 64)


def test_cpu_tensors_are_rejected_loudly():
    from nicr_mt_scene_analysis_amd import ops
    with pytest.raises(L.NmsaError):
        ops.semantic_argmax(torch.zeros((1, 3, 4, 4)))


def test_raw_pointer_helper_refuses_pageable_host_memory():
    """`_lib.ptr` is the one place a tensor becomes a kernel argument: a pageable host tensor
    there would be a GPU memory fault (a test of round 5 did exactly that), so it raises"""
    with pytest.raises(ValueError, match='pageable'):
        L.ptr(torch.zeros(8))
    assert L.ptr(None) is None


def test_header_is_plain_c99():
    """include/nmsa.h is the FFI contract: it must compile as C (no C++ / HIP types)."""
    import os
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        import pytest
        pytest.skip('no gcc')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([gcc, '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror',
                           '-fsyntax-only', '-x', 'c', os.path.join(root, 'include', 'nmsa.h')])
