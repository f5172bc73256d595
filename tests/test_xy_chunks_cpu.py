"""The partition of the chunked x <-> y pair of the fused SENSE leaf (indigo_amd/csrc/ig_fft_xy.h), on the host: no GPU.

exec_padded / exec_cropped of ig_fft_plan.hip launch what this header hands them: chunk i covers planes [z0 + i K, ...) on stream
i mod S.  tools/xy_chunks_check.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers, walks it for
every number of planes 1 ... 300, K = 0 ... planes + 1 and S = 1 ... 3: the chunks tile [z0, z1) exactly once, none is empty, and
stream indices stay below S."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def test_partition_tiles_every_range_under_the_sanitizers(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "xy_chunks_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "xy_chunks_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, "300"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    # planes 1 ... 300, K 0 ... planes + 1, S 1 ... 3, two origins
    assert r.stdout.startswith("ok %d partitions up to 300 planes" % (sum(p + 2 for p in range(1, 301)) * 3 * 2)), r.stdout
