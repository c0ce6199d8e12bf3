"""Host side of the item-based job's remaining options (usersFile, itemsFile, ratingShift, outputPathForSimilarityMatrix): the
id-file reader, the text writer of the item pairs, the layout of fy_itemcf_filter and the argument plumbing.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID_FILE = b"3\n\n  \nabc\n12x\n-7\n 41 \n+5\n2147483647\n2147483648\n-2147483648\n-2147483649\n99999999999999999999999\n1.5\n- 3\n-\n8\r\n3\n17"
ID_WANT = [3, -7, 41, 5, 2147483647, -2147483648, 8, 3, 17]


def test_id_file_skips_what_is_not_an_int32(tmp_path):
    """Blank lines, `abc`, `12x`, values beyond int32 on either side, a sign alone, CRLF, a duplicate (kept: the set is made on the
    device) and a last line without a newline."""
    P = pkg()
    p = tmp_path / "users.txt"
    p.write_bytes(ID_FILE)
    ids = P.read_id_file(str(p))
    assert ids.dtype == np.int32 and ids.tolist() == ID_WANT
    empty = tmp_path / "empty.txt"
    empty.write_bytes(b"")
    assert P.read_id_file(empty).tolist() == []
    with pytest.raises(P.FilmYouError) as e:
        P.read_id_file(str(tmp_path / "missing.txt"))
    assert e.value.code == -12
    lib = P._native.load()
    assert lib.fy_idfile_read(None, None, None) == -1


def test_pairs_text_round_trips_the_floats(tmp_path):
    P = pkg()
    rng = np.random.default_rng(5)
    sim = np.concatenate([np.array([0.5, 1.0, 0.1, 1e-30, 3.4028235e38, 0.0, -0.25, 1 / 3], dtype=np.float32),
                          rng.random(2000).astype(np.float32)])
    a = np.arange(len(sim), dtype=np.int32) + 1
    b = a + 7
    out = tmp_path / "deep" / "dir" / "pairs.txt"
    P.write_similarity_pairs(str(out), {"a": a, "b": b, "sim": sim})
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == len(sim) + 1
    assert lines[0] == "1\t8\t0.5" and lines[1] == "2\t9\t1"
    assert lines[2] == "3\t10\t0.10000000149011612"          # the float widened to double, not "0.1"
    for k, line in enumerate(lines[:-1]):
        x, y, v = line.split("\t")
        assert (int(x), int(y)) == (int(a[k]), int(b[k]))
        assert float(v) == float(sim[k]) and np.float32(float(v)) == sim[k]
        # the shortest: one digit fewer no longer reads back
        digits = len(v.split("e")[0].replace("-", "").replace(".", "").lstrip("0"))
        if digits > 1:
            assert float("%.*g" % (digits - 1, float(sim[k]))) != float(sim[k])
    lib = P._native.load()
    assert lib.fy_simpairs_write_text(None, 0, None, None, None) == -1
    assert lib.fy_simpairs_write_text(str(out).encode(), 3, None, None, None) == -1


def test_filter_struct_and_abi_version():
    P = pkg()
    N = P._native
    assert C.sizeof(N.ItemCFFilter) == 40
    assert [(f, getattr(N.ItemCFFilter, f).offset) for f, _ in N.ItemCFFilter._fields_] == [
        ("has_users", 0), ("has_items", 4), ("n_users", 8), ("users", 16), ("n_items", 24), ("items", 32)]
    assert C.sizeof(N.ItemCFParams) == 24 and N.load().fy_abi_version() == 5
    for name in ("fy_itemcf_recommend_filtered", "fy_ratings_shifted", "fy_itemsim_pairs", "fy_simpairs_write_text", "fy_idfile_read"):
        assert name in N.SYMBOLS and hasattr(N.load(), name)


def test_argument_validation_without_a_device():
    P = pkg()
    lib = P._native.load()
    out = C.c_void_p(1)
    p = P._native.ItemCFParams(10, 50, 0, 0, 1, 0)
    f = P._native.ItemCFFilter(1, 0, 0, None, 0, None)
    assert lib.fy_itemcf_recommend_filtered(None, C.byref(p), C.byref(f), None, None, C.byref(out)) == -1
    assert out.value is None and b"NULL" in lib.fy_last_error()
    assert lib.fy_itemcf_recommend_filtered(None, C.byref(p), C.byref(f), None, None, None) == -1
    out = C.c_void_p(1)
    assert lib.fy_ratings_shifted(None, None, 1.0, C.byref(out)) == -1 and out.value is None
    out = C.c_void_p(1)
    assert lib.fy_itemsim_pairs(None, None, C.byref(out)) == -1 and out.value is None


def test_job_keywords_and_id_lists(tmp_path):
    P = pkg()
    sig = inspect.signature(P.BaselineRecommenderJob.run)
    assert sig.parameters["usersFile"].default is None and sig.parameters["itemsFile"].default is None
    assert sig.parameters["ratingShift"].default == 0.0 and sig.parameters["outputPathForSimilarityMatrix"].default is None
    assert hasattr(P.Ratings, "shifted") and hasattr(P.ItemSimilarities, "pairs")
    host = __import__("importlib").import_module("filmyou-core_amd.host")
    p = tmp_path / "items.txt"
    p.write_bytes(ID_FILE)
    assert host._id_list(None) is None
    assert host._id_list(str(p)).tolist() == ID_WANT and host._id_list(p).tolist() == ID_WANT
    got = host._id_list([4, 4, 9])
    assert got.dtype == np.int32 and got.tolist() == [4, 4, 9]
    assert host._id_list(np.zeros(0, dtype=np.int64)).tolist() == []


def test_cpp_mirror_names_the_four_options(tmp_path):
    """The C++ mirror (host/filmyou_job.hpp) carries the same four options and still compiles on its own."""
    hdr = os.path.join(ROOT, "filmyou-core_amd", "host", "filmyou_job.hpp")
    text = open(hdr).read()
    for word in ("usersFile", "itemsFile", "ratingShift", "outputPathForSimilarityMatrix", "fy_itemcf_recommend_filtered"):
        assert word in text, word
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "filmyou_job.hpp"\nint main() { fy::host::BaselineRecommenderJob job; return job.numRecommendations == 100 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(hdr), str(src)], check=True)


def test_id_file_and_pair_writer_under_asan_ubsan(tmp_path):
    """The new host code of csrc/fy_seqfile.cpp under ASan + UBSan, like the codec in test_sanitizers_cpu.py."""
    out = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not out or not os.path.isabs(out) or not os.path.exists(out):
        pytest.skip("libasan.so is not installed")
    (tmp_path / "ids.txt").write_bytes(ID_FILE)
    drv = tmp_path / "drv.cpp"
    drv.write_text(r'''
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "filmyou.h"
int main(int argc, char** argv) {
    const std::string dir = argv[1];
    int64_t n = 0;
    int32_t* ids = nullptr;
    if (fy_idfile_read((dir + "/ids.txt").c_str(), &n, &ids)) return 1;
    long long sum = 0;
    for (int64_t i = 0; i < n; i++) sum += ids[i];
    fy_buffer_free(ids);
    if (fy_idfile_read((dir + "/none.txt").c_str(), &n, &ids) == 0) return 2;
    std::vector<int32_t> a(1000), b(1000);
    std::vector<float> s(1000);
    for (int i = 0; i < 1000; i++) { a[i] = i; b[i] = i + 1; s[i] = 1.0f / (float)(i + 1); }
    s[7] = 3.4028235e38f; s[8] = 1e-45f; s[9] = 0.0f;
    if (fy_simpairs_write_text((dir + "/sub/pairs.txt").c_str(), 1000, a.data(), b.data(), s.data())) return 3;
    printf("ok %lld %lld\n", (long long)n, sum);
    return 0;
}
''')
    stub = tmp_path / "stub.cpp"
    stub.write_text(r'''
#include <cstdarg>
#include <cstdio>
namespace fy { void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc(10, stderr); }
               const char* last_error() { return ""; } }
''')
    exe = str(tmp_path / "drv")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                    "-I", os.path.join(ROOT, "include"), "-o", exe, str(drv), str(stub),
                    os.path.join(ROOT, "filmyou-core_amd", "csrc", "fy_seqfile.cpp")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d %d" % (len(ID_WANT), sum(ID_WANT)))
