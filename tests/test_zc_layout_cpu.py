"""The address map of the z-contiguous y <-> z intermediate (indigo_amd/csrc/ig_fft_zc.h), on the host: no GPU.

ig_fft_zc_offset / ig_fft_zc_size are the map the pass schedule of ig_fft_plan.hip is built from.  Checked here through the library
on the planes where an error would show (first, second and last ky and z, every (kx, coil)), and in full -- every element of
every shape, both passes walked the way the kernel's workgroups address them -- by tools/zc_layout_check.cpp, a stand-alone
program built with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (grid, image box) of tests/test_hip_zc_intermediate.py, and the headline's; tile widths: 32 columns on a 512-point axis, else 16
SHAPES = [((256, 256, 256), (128, 128, 128)),
          ((256, 256, 256), (160, 160, 160)),
          ((512, 256, 256), (256, 128, 128)),
          ((256, 256, 512), (128, 128, 256))]
HEADLINE = ((512, 512, 512), (256, 256, 256))
COILS = [8, 4, 2]


def _width(n):
    return 32 if n == 512 else 16


def _lo(grid, box):
    return tuple(m // 2 + int(np.ceil(-n / 2)) for m, n in zip(grid, box))


@pytest.fixture(scope="module")
def L():
    from indigo_amd._lib import lib
    return lib()


def _a3(v):
    return (ctypes.c_int64 * 3)(*v)


@pytest.mark.parametrize("coils", COILS)
@pytest.mark.parametrize("grid,box", SHAPES + [HEADLINE])
def test_offsets_are_distinct_in_range_and_z_contiguous(L, grid, box, coils):
    n0, n1, n2 = grid
    b2 = box[2]
    piece = _width(n2) * 8
    g, b = _a3(grid), _a3(box)
    size = L.ig_fft_zc_size(g, b, coils, piece)
    assert size == n0 * n1 * b2 * coils * 8
    assert size <= n0 * n1 * n2 * coils * 8, "never more than the full-size array it replaces"
    kys, zs = sorted({0, 1, n1 // 2, n1 - 1}), sorted({0, 1, b2 - 1})
    kxs = range(n0) if grid != HEADLINE[0] else list(range(0, 64)) + list(range(n0 - 64, n0))
    off = np.array([[[[L.ig_fft_zc_offset(g, b, coils, piece, kx, ky, z, c) for c in range(coils)] for kx in kxs] for z in zs] for ky in kys],
                   dtype=np.int64)                                        # [ky, z, kx, c]
    assert off.min() >= 0 and off.max() <= size - 8 and (off % 8 == 0).all()
    assert np.unique(off).size == off.size, "two elements share an address"
    # a piece: `piece` bytes of consecutive (c, kx), contiguous; the next z of the same columns follows right behind it, the next
    # ky after box_z of them
    flat = off.reshape(len(kys), len(zs), -1)                             # (c, kx) combined, c fastest
    cols = piece // 8
    tiles = flat.reshape(len(kys), len(zs), -1, cols)
    assert (np.diff(tiles, axis=3) == 8).all() and (tiles[..., 0] % piece == 0).all()
    assert (flat[:, 1] - flat[:, 0] == piece).all(), "z neighbours of a tile are adjacent pieces"
    assert (flat[:, len(zs) - 1] - flat[:, 0] == (b2 - 1) * piece).all(), "a z tile is one run of box_z pieces"
    assert (flat[1] - flat[0] == b2 * piece).all(), "ky neighbours: one run apart"
    # outside the geometry
    assert L.ig_fft_zc_offset(g, b, coils, piece, n0, 0, 0, 0) == -1 and L.ig_fft_zc_offset(g, b, coils, piece, 0, 0, b2, 0) == -1
    assert L.ig_fft_zc_offset(g, b, coils, piece, 0, n1, 0, 0) == -1 and L.ig_fft_zc_offset(g, b, coils, piece, 0, 0, 0, coils) == -1
    assert L.ig_fft_zc_size(g, b, coils, 24) == -1


def test_map_is_a_bijection_for_a_whole_small_geometry(L):
    """every element of a grid small enough to enumerate through the library: 32 x 8 x 16, box 6 planes, 2 coils, 128-byte pieces"""
    grid, box, C = (32, 8, 16), (16, 4, 6), 2
    g, b = _a3(grid), _a3(box)
    size = L.ig_fft_zc_size(g, b, C, 128)
    off = sorted(L.ig_fft_zc_offset(g, b, C, 128, kx, ky, z, c) for kx in range(32) for ky in range(8) for z in range(6) for c in range(C))
    assert off == list(range(0, size, 8))


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def test_pass_schedule_walks_the_array_under_the_sanitizers(tmp_path):
    """tools/zc_layout_check.cpp with -fsanitize=address,undefined: both passes of every shape and coil count, every element"""
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "zc_layout_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "zc_layout_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    procs = []                                           # one process per shape, side by side
    for grid, box in SHAPES:
        args = []
        for C in COILS:
            args += [grid[0], grid[1], grid[2], box[2], _lo(grid, box)[2], C, _width(grid[1]), _width(grid[2])]
        procs.append(subprocess.Popen([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for pr in procs:
        out = pr.communicate()[0]
        assert pr.returncode == 0, out
        assert out.count("ok ") == len(COILS), out
    # a geometry the route refuses -- a y tile wider than a piece -- is refused here too
    r = subprocess.run([exe, "512", "512", "256", "128", "64", "8", "32", "16"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 1 and "bad geometry" in r.stdout
