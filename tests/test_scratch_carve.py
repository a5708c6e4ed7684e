"""CPU check of the scratch carver's sizing core (csrc/scratch_core.h): a stand-alone C++ program, built
with the system g++ under AddressSanitizer and UBSan, carves host blocks of exactly the measured size and
writes every byte of every region. Nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrosion_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scratch_core.h"

using corro::Carver;

struct E16 { uint64_t a, b; };
static const size_t ES[4] = {1, 4, 8, 16};
static const size_t CS[11] = {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257};

static int copies = 0;
static bool copy_to(void *, void *dst, const void *src, size_t bytes) {
    copies++;
    std::memcpy(dst, src, bytes);                  // (ASan: inside the block, inside the source)
    return true;
}

#define CHECK(x)                                                               \
    do {                                                                       \
        if (!(x)) {                                                            \
            std::fprintf(stderr, "%s:%d: %s (layout %d)\n", __FILE__, __LINE__, #x, layouts); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static uint8_t *take(Carver &c, size_t elem, size_t count) {
    switch (elem) {
    case 1: return c.take<uint8_t>(count);
    case 4: return reinterpret_cast<uint8_t *>(c.take<uint32_t>(count));
    case 8: return reinterpret_cast<uint8_t *>(c.take<uint64_t>(count));
    default: return reinterpret_cast<uint8_t *>(c.take<E16>(count));
    }
}

int main() {
    int layouts = 0;
    for (int nreg = 1; nreg <= 6; nreg++)
        for (int ei = 0; ei < 4; ei++)
            for (int ci = 0; ci < 11; ci++)
                for (int stride = 1; stride <= 5; stride += 2)
                    for (int staged = 0; staged < 2; staged++) {
                        layouts++;
                        size_t elem[6], count[6];
                        for (int j = 0; j < nreg; j++) {
                            elem[j] = ES[(ei + j) % 4];
                            count[j] = CS[(ci + j * stride) % 11];
                        }
                        // one host array staged behind the regions, with 16 bytes of padding room
                        const size_t sbytes = count[0] * elem[0];
                        std::vector<uint8_t> src(sbytes, 0x5A);
                        const uint8_t *srcp = src.data();

                        uint8_t *ptr[6] = {};
                        const uint8_t *staged_at = nullptr;
                        size_t end_used[2] = {~(size_t)0, ~(size_t)0};
                        int calls = 0, copies_measuring = -1;
                        bool zero_ok = true;
                        copies = 0;
                        auto layout = [&](Carver &c) {
                            for (int j = 0; j < nreg; j++) {
                                const size_t before = c.used;
                                ptr[j] = take(c, elem[j], count[j]);
                                if (count[j] == 0 && c.used != before) zero_ok = false;
                                if (count[j] != 0 && c.used != before + corro::al256(count[j] * elem[j])) zero_ok = false;
                            }
                            staged_at = c.up(srcp, sbytes, sbytes + 16);
                            if (!c.live) copies_measuring = copies;
                            end_used[c.live ? 1 : 0] = c.used;
                            calls++;
                        };
                        uint8_t *block = nullptr;
                        size_t block_bytes = 0;
                        int ensures = 0;
                        auto ensure = [&](size_t want, uint8_t **base) {
                            ensures++;
                            block_bytes = want;
                            block = static_cast<uint8_t *>(std::malloc(want));   // exactly the measured size
                            *base = block;
                            return 0;
                        };
                        bool copies_ok = true;
                        const int rc = corro::carve_with(ensure, layout, staged ? copy_to : nullptr, nullptr, &copies_ok);
                        CHECK(rc == 0 && copies_ok);
                        CHECK(calls == 2 && ensures == 1);                       // measured once, carved once
                        CHECK(copies_measuring == 0);                            // the measuring pass copies nothing
                        CHECK(end_used[0] == block_bytes && end_used[1] == block_bytes);
                        CHECK(zero_ok);
                        CHECK(block != nullptr || block_bytes == 0);
                        for (int j = 0; j < nreg; j++) {
                            const size_t at = (size_t)(ptr[j] - block);
                            CHECK(ptr[j] >= block && at <= block_bytes);         // inside, or one past (an empty tail)
                            CHECK(at % 256 == 0);
                            if (j + 1 < nreg) CHECK(ptr[j] + count[j] * elem[j] <= ptr[j + 1]);
                            else CHECK(at + count[j] * elem[j] <= block_bytes);
                            if (count[j]) std::memset(ptr[j], 0xA0 + j, count[j] * elem[j]);   // (ASan is the judge)
                        }
                        for (int j = 0; j < nreg; j++)                            // no region wrote into another
                            for (size_t k = 0; k < count[j] * elem[j]; k++) CHECK(ptr[j][k] == 0xA0 + j);
                        if (staged) {
                            CHECK(copies == (sbytes ? 1 : 0));
                            const size_t at = (size_t)(staged_at - block);
                            CHECK(at % 256 == 0 && at + sbytes + 16 <= block_bytes);
                            CHECK(nreg == 0 || ptr[nreg - 1] + count[nreg - 1] * elem[nreg - 1] <= staged_at);
                            for (size_t k = 0; k < sbytes; k++) CHECK(staged_at[k] == 0x5A);
                            std::memset(const_cast<uint8_t *>(staged_at), 1, sbytes + 16);
                        } else {
                            CHECK(copies == 0 && staged_at == srcp);             // device arrays are handed through
                        }
                        std::free(block);
                    }
    // a failed copy is sticky and reported; a failed ensure ends the carve before the live pass
    {
        int calls = 0;
        uint8_t one = 0;
        auto layout = [&](Carver &c) {
            calls++;
            (void)c.up(&one, 1, 1);
            (void)c.up(&one, 1, 1);
        };
        std::vector<uint8_t> block;
        auto ensure = [&](size_t want, uint8_t **base) {
            block.resize(want);
            *base = block.data();
            return 0;
        };
        int n = 0;
        struct Fail {
            static bool first(void *arg, void *, const void *, size_t) { return (*static_cast<int *>(arg))++ != 0; }
        };
        bool copies_ok = true;
        CHECK(corro::carve_with(ensure, layout, &Fail::first, &n, &copies_ok) == 0);
        CHECK(!copies_ok && n == 2 && calls == 2);
        calls = 0;
        auto refuse = [&](size_t, uint8_t **) { return -5; };
        CHECK(corro::carve_with(refuse, layout) == -5 && calls == 1);
    }
    std::printf("ok %d\n", layouts);
    return 0;
}
"""


def test_carver_measures_what_it_carves_under_asan_and_ubsan():
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="corro_scratch_carve_")
    try:
        src, exe = os.path.join(d, "carve.cpp"), os.path.join(d, "carve")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                               "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe])
        res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert res.returncode == 0, res.stderr.decode()[-4000:]
    assert res.stdout.decode().split() == ["ok", str(6 * 4 * 11 * 3 * 2)]


def test_sizing_core_includes_no_hip_header():
    with open(os.path.join(CSRC, "scratch_core.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and '#include "internal.h"' not in text
