"""Caller-owned scratch (csrc/workspace.hpp: the bump Carver and check_workspace), compiled for the host into a small stand-alone
program that answers one query per input line.  No GPU: the entry points and this test share the one copy of the code.

NGP_WORKSPACE_TEST_CXXFLAGS adds compiler flags; with "-fsanitize=address,undefined -fno-sanitize-recover=all" the program -- which has
its own main and writes every byte of every region it carves -- runs under the sanitizers with nothing preloaded."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerfsafetyvalidation_amd", "csrc")
SIZE_MAX = (1 << 64) - 1
NGP_OK, NGP_EINVAL, NGP_EWORKSPACE = 0, -1, -3

MAIN = r"""
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "workspace.hpp"

static char g_err[256];
namespace ngp {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace ngp
using namespace ngp;

struct alignas(16) Vec16 { unsigned char b[16]; };
struct Op { char kind; size_t size, count, align; };      // 't'ake (align 0: the type's own) or 'p'ad (count bytes)

template <typename T>
static char* take(Carver& c, const Op& o) { return reinterpret_cast<char*>(o.align ? c.take<T>(o.count, o.align) : c.take<T>(o.count)); }
static char* apply(Carver& c, const Op& o) {
    if (o.kind == 'p') { c.pad(o.count); return nullptr; }
    switch (o.size) {
        case 1: return take<uint8_t>(c, o);
        case 2: return take<uint16_t>(c, o);
        case 4: return take<uint32_t>(c, o);
        case 8: return take<double>(c, o);
        default: return take<Vec16>(c, o);
    }
}

// "layout carve|measure  t:size:count:align | p:bytes ..." -> per take "offset_measured offset_carved", then "bytes_measured bytes_carved"
// (carved values -1 with `measure`).  Carving runs over a heap block of exactly bytes() bytes, `skew` bytes into a 64-byte line; every
// region is filled with its index and read back, so a region that leaves the block or overlaps another shows here and under ASan.
static void layout(char* line) {
    std::vector<Op> ops;
    char mode[16];
    unsigned skew = 0;
    int used = 0;
    sscanf(line, "%15s %u%n", mode, &skew, &used);
    for (char* tok = strtok(line + used, " \n"); tok; tok = strtok(nullptr, " \n")) {
        Op o = {tok[0], 0, 0, 0};
        if (o.kind == 't') sscanf(tok, "t:%zu:%zu:%zu", &o.size, &o.count, &o.align);
        else sscanf(tok, "p:%zu", &o.count);
        ops.push_back(o);
    }
    Carver m;
    std::vector<size_t> before;
    for (const Op& o : ops) {
        apply(m, o);
        before.push_back(m.bytes());
    }
    const bool carve = !strcmp(mode, "carve");
    char* block = nullptr;
    std::vector<char*> ptr(ops.size(), nullptr);
    size_t carved_bytes = 0;
    if (carve) {
        block = static_cast<char*>(malloc(m.bytes() + skew ? m.bytes() + skew : 1));
        Carver c(block + skew);
        for (size_t i = 0; i < ops.size(); i++) {
            ptr[i] = apply(c, ops[i]);
            if (ops[i].kind == 't') memset(ptr[i], (int)(i + 1), ops[i].size * ops[i].count);
        }
        carved_bytes = c.bytes();
        for (size_t i = 0; i < ops.size(); i++)
            for (size_t k = 0; ops[i].kind == 't' && k < ops[i].size * ops[i].count; k++)
                if ((unsigned char)ptr[i][k] != (unsigned char)(i + 1)) { printf("overlap\n"); free(block); return; }
    }
    for (size_t i = 0; i < ops.size(); i++) {
        if (ops[i].kind != 't') continue;
        const size_t end = before[i], bytes = ops[i].size > SIZE_MAX / (ops[i].count ? ops[i].count : 1) ? 0 : ops[i].size * ops[i].count;
        printf("%zu %lld ", end == SIZE_MAX ? SIZE_MAX : end - bytes, carve ? (long long)(ptr[i] - (block + skew)) : -1ll);
    }
    printf("%zu %lld\n", m.bytes(), carve ? (long long)carved_bytes : -1ll);
    free(block);
}

int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "layout ", 7)) {
            layout(line + 7);
        } else {      // "check pointer given need align" -> "rc|message"
            size_t p, given, need, align;
            sscanf(line, "check %zu %zu %zu %zu", &p, &given, &need, &align);
            strcpy(g_err, "-");
            const int rc = check_workspace("entry_point", reinterpret_cast<const void*>(p), given, need, align);
            printf("%d|%s\n", rc, g_err);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("workspace")
    src, exe = d / "main.cpp", d / "workspace"
    src.write_text(MAIN)
    extra = shlex.split(os.environ.get("NGP_WORKSPACE_TEST_CXXFLAGS", ""))
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-o", str(exe), str(src)])

    def run(lines):
        done = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-2000:]
        rows = done.stdout.splitlines()
        assert len(rows) == len(lines), done.stdout[-2000:]
        return rows
    return run


def model(ops):
    """the offsets a bump allocator gives: round up to the alignment, hand out, advance; saturating at SIZE_MAX"""
    off, starts = 0, []
    for op in ops:
        if op[0] == "p":
            off = min(SIZE_MAX, off + op[1])
            continue
        _, size, count, align = op
        align = align or size
        off = min(SIZE_MAX, (off + align - 1) // align * align)
        starts.append(off)
        off = min(SIZE_MAX, off + size * count)
    return starts, off


def spell(ops):
    return " ".join(f"p:{op[1]}" if op[0] == "p" else "t:%d:%d:%d" % op[1:] for op in ops)


# layouts in the shapes the entry points use: mixed element sizes, explicit alignment, pads, empty regions, odd counts
LAYOUTS = [
    [("t", 4, 5, 0), ("t", 4, 1, 0), ("t", 4, 2, 0), ("p", 8), ("t", 1, 4096, 16), ("t", 1, 512, 0), ("t", 8, 5 * 16, 0)],      # the train march
    [("t", 8, 2, 0), ("t", 2, 210, 8), ("t", 2, 210, 8), ("t", 1, 210, 8), ("t", 1, 210, 0), ("t", 1, 210, 0), ("p", 64)],      # the isosurface, 5 x 6 x 7
    [("t", 4, 1, 0), ("p", 60), ("t", 4, 210, 0), ("t", 4, 1, 0)],                                                              # the components
    [("t", 8, 64, 0), ("t", 8, 8, 0), ("p", 64)],                                                                              # the density grid, H = 4 x 8
    [("t", 1, 3, 0), ("t", 8, 1, 0), ("t", 1, 1, 0), ("t", 2, 3, 0), ("t", 16, 2, 0), ("t", 1, 7, 0), ("t", 4, 0, 0), ("t", 8, 0, 64), ("t", 1, 1, 0)],
    [("t", 4, 0, 0)],
    [],
]


@pytest.mark.parametrize("skew", [0, 16, 64])
def test_measuring_and_carving_agree_and_regions_are_aligned_disjoint_and_inside(ask, skew):
    """(the base is 16-byte aligned for skew 16 and more for the others; no layout above asks for more than its base has, but for
    the one 64-byte take, which only skew 0 and 64 can honour absolutely -- relative to the base every skew must)"""
    rows = ask([f"layout carve {skew} {spell(ops)}" for ops in LAYOUTS])
    for ops, row in zip(LAYOUTS, rows):
        assert row != "overlap", ops
        vals = [int(v) for v in row.split()]
        measured, carved, (bytes_m, bytes_c) = vals[0:-2:2], vals[1:-2:2], vals[-2:]
        starts, total = model(ops)
        assert measured == carved == starts and bytes_m == bytes_c == total, (ops, row)
        takes = [op for op in ops if op[0] == "t"]
        spans = []
        for (_, size, count, align), start in zip(takes, starts):
            assert start % (align or size) == 0, (ops, start)
            assert start + size * count <= total
            if count:
                spans.append((start, start + size * count))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (ops, spans)


def test_offsets_do_not_wrap_near_half_the_address_space_and_saturate_at_the_top(ask):
    half = SIZE_MAX // 2
    big = [
        [("t", 1, half - 5, 0), ("t", 8, 3, 0), ("t", 4, 7, 0)],                  # crosses SIZE_MAX / 2: plain sums, no sign trouble
        [("t", 8, half // 8, 0), ("t", 8, half // 8 - 8, 0), ("t", 1, 1, 16)],      # ends just below SIZE_MAX
        [("t", 8, half // 4 + 1, 0), ("t", 4, 1, 0)],                             # count * sizeof(T) itself overflows: saturates
        [("t", 1, SIZE_MAX - 3, 0), ("t", 8, 1, 0)],                              # the rounding-up would wrap: saturates
        [("t", 1, SIZE_MAX - 3, 0), ("p", 4), ("t", 1, 1, 0)],                    # the pad would wrap: saturates
        [("t", 4, (1 << 31) - 1, 0), ("t", 2, (1 << 31) - 1, 0), ("t", 2, (1 << 31) - 1, 0), ("p", 64)],      # 2^31 - 1 cells of the EDT
    ]
    rows = ask([f"layout measure 0 {spell(ops)}" for ops in big])
    totals = []
    for ops, row in zip(big, rows):
        vals = [int(v) for v in row.split()]
        starts, total = model(ops)
        assert vals[-2] == total and vals[-1] == -1, (ops, row)
        if total != SIZE_MAX:
            assert vals[0:-2:2] == starts, (ops, row)
        totals.append(total)
    assert totals[0] == (half + 1) + 24 + 28 and half < totals[1] < SIZE_MAX and totals[2:5] == [SIZE_MAX] * 3
    assert totals[5] == 8 * ((1 << 31) - 1) + 64


def test_check_workspace_takes_every_branch(ask):
    aligned, odd = 0x7000_0000_1000, 0x7000_0000_1004
    rows = ask([
        "check 0 0 0 8",                    # nothing needed: NULL is fine
        f"check {odd} 3 0 8",               # ... and so is anything else
        f"check {aligned} 4096 4096 8",     # exactly enough
        f"check {aligned} 4095 4096 8",     # one byte short
        "check 0 0 4096 8",                 # no workspace at all: too small, by name
        f"check {odd} 100 4096 8",          # too small wins over misaligned
        "check 0 4096 4096 8",              # enough bytes claimed behind NULL
        f"check {odd} 4096 4096 8",         # misaligned for 8
        f"check {odd} 4096 4096 4",         # aligned for 4
        f"check {aligned} {SIZE_MAX - 1} {SIZE_MAX} 16",      # a saturated layout: nothing satisfies it
    ])
    got = [(int(r.split("|")[0]), r.split("|", 1)[1]) for r in rows]
    assert [rc for rc, _ in got] == [NGP_OK, NGP_OK, NGP_OK, NGP_EWORKSPACE, NGP_EWORKSPACE, NGP_EWORKSPACE, NGP_EINVAL, NGP_EINVAL, NGP_OK,
                                     NGP_EWORKSPACE]
    assert all(msg == "-" for rc, msg in got if rc == NGP_OK)          # a pass leaves ngp_last_error() alone
    assert got[3][1] == "entry_point: workspace too small (4095 < 4096 bytes)"
    assert got[4][1] == "entry_point: workspace too small (0 < 4096 bytes)"
    assert got[9][1] == f"entry_point: workspace too small ({SIZE_MAX - 1} < {SIZE_MAX} bytes)"
    for rc, msg in got:
        if rc == NGP_EINVAL:
            assert msg.startswith("entry_point: workspace is NULL or not 8-byte aligned"), msg


IN_SCOPE = ["raymarching.hip", "collision.hip", "components.hip", "mesh.hip", "closest.hip", "render_uniform.hip", "density_grid.hip", "capi.hip",
            "sigma_fit.hip", "image_metrics.hip", "features.hip", "train_data.hip", "distortion.hip", "depth_loss.hip", "ngp_common.hpp"]


def test_no_entry_point_casts_its_workspace_or_words_its_own_refusal():
    """The layout functions see a Carver, never the pointer: so in the files whose workspaces go through workspace.hpp nothing casts
    `workspace` at all, and the text of the refusal exists once, in the header."""
    cast = re.compile(r"reinterpret_cast\s*<[^>]*>\s*\(\s*workspace\b|static_cast\s*<[^>]*>\s*\(\s*workspace\b|\*\s*\)\s*workspace\b|uintptr_t\s*\)\s*workspace\b")
    for name in IN_SCOPE:
        text = open(os.path.join(CSRC, name)).read()
        found = [ln for ln in text.splitlines() if cast.search(ln)]
        assert not found, (name, found)
        assert "workspace too small" not in text, name
    assert open(os.path.join(CSRC, "workspace.hpp")).read().count('"%s: workspace too small (%zu < %zu bytes)"') == 1
