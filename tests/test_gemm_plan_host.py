"""Which kernel, tile form and split-K factor a GEMM shape gets (csrc/gemm_plan.h), checked on the host against a recorded table.

tests/golden/gemm_dispatch.json holds 13 000 cases in blocks ``[planner, [values per input column], [answers]]``: the cases of
a block are the cartesian product of its value lists, each answer an index into the file's table of distinct plans.  The answers were recorded
from the launchers of the commit BEFORE gemm_plan.h existed, not from the planner: a throw-away copy of that commit's
gemm_nt.hip, gemm_nt256.hip, gemm_tn.hip and gemm_tn256.hip (built with -DSMD_TN_EXPERIMENTS so that every kernel variant
exists) was compiled host-only with ``hipLaunchKernelGGL`` redefined, behind the includes, to record the kernel
instantiation, grid, block, dynamic-LDS bytes and integer arguments, and ``hipGetLastError`` stubbed to success; a small
``main`` set the knobs with smd_tuning_set and drove launch_gemm_nt (behind SmdEngine::dense_fwd's min_tiles rule),
launch_gemm_tn, launch_gemm_tn_grouped and launch_gemm_tn256_multi with dummy pointers over
  * every GEMM the engine issues (SmdEngine::dense_fwd, dense_bwd, wgrad) at the data widths of the configurations -- C = 42 (mel,
    padded to 64), 146 (multi, padded to 192) and the benchmark's 512 -- for batch 256 and 64, forward, backward, sampling with one
    and two chains and 1000 sequences at once, FiLM tables; and the problem lists SmdEngine::flush_grouped_wgrads hands to
    launch_gemm_tn_grouped (FiLM generators of 2 / 3 blocks, out_proj + up, an encoder layer, layer 0 + in_proj, everything at the
    end) with the engine's slab workspace,
  * a grid around every threshold of the rules, under the default knobs and under every non-default knob value the tests and
    tools/kbench.py set.
That recorder is not part of the repository.  Here a stand-alone program (tests/gemm_plan_dump.cpp, which includes only
gemm_plan.h) is built with the host compiler and -fsanitize=address,undefined, reads the table and prints the planners'
answers; they must equal the recorded ones exactly.
"""
import collections
import itertools
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "symbolic-music-diffusion_amd", "csrc")
TABLE = os.path.join(HERE, "golden", "gemm_dispatch.json")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    pytest.fail("no host C++ compiler found (looked at $CXX, g++, c++, clang++)")


@pytest.fixture(scope="module")
def table():
    """The recorded cases, expanded: {"inputs": columns per planner, "rows": [planner, inputs..., recorded answer...]}."""
    with open(TABLE) as f:
        doc = json.load(f)
    rows, inputs = [], {}
    for planner, values, answers in doc["blocks"]:
        cases = list(itertools.product(*values))
        assert len(cases) == len(answers)
        inputs[planner] = len(values)
        rows += [[planner, *case, *doc["plans"][planner][a]] for case, a in zip(cases, answers)]
    return {"inputs": inputs, "rows": rows}


@pytest.fixture(scope="module")
def answers(table, tmp_path_factory):
    """The planners' answers for every row of the table, from the sanitized stand-alone program."""
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "gemm_plan_dump.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, TABLE], check=True, capture_output=True, text=True)
    assert r.stderr == "", r.stderr
    return [line.split() for line in r.stdout.splitlines()]


def test_gemm_plan_header_stands_alone():
    """Plain C++17, no HIP include: the header compiles on its own with the host compiler."""
    subprocess.run([_cxx(), "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "gemm_plan.h")], check=True)
    with open(os.path.join(CSRC, "gemm_plan.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "smd_tuning_get(" not in text      # the launchers read the knobs and pass the values in


def test_planners_answer_what_the_launchers_launched(table, answers):
    rows = table["rows"]
    assert len(answers) == len(rows)
    wrong = []
    for row, got in zip(rows, answers):
        n_in = table["inputs"][row[0]]
        if got[0] != row[0] or [int(x) for x in got[1:]] != row[1 + n_in:]:
            wrong.append((row, got))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ, first: {wrong[:5]}"


def test_table_reaches_every_branch(table):
    """The table cannot pass by covering the easy cases only: distinct recorded plans are counted against the branches."""
    by = collections.defaultdict(list)
    for row in table["rows"]:
        by[row[0]].append(row)
    n = table["inputs"]
    nt = by["nt"]
    out = lambda r, tag: r[1 + n[tag]:]
    # nt_plan: all ten (kernel, BM, NS, KG) forms, each epilogue flag both ways on the kernel that has it
    forms = {tuple(out(r, "nt")[:4]) for r in nt}
    assert forms == {(128, 32, 2, 1), (128, 32, 4, 1), (128, 32, 3, 2), (128, 64, 2, 1), (128, 64, 2, 2), (128, 64, 3, 2),
                     (128, 128, 2, 1), (128, 128, 2, 2), (128, 128, 3, 1), (256, 256, 2, 1)}
    assert {(out(r, "nt")[0], out(r, "nt")[6]) for r in nt} >= {(256, 0), (256, 1)}          # packed-bf16 epilogue
    assert {(out(r, "nt")[0], out(r, "nt")[7]) for r in nt} >= {(128, 0), (128, 1)}          # vector epilogue
    default = [1, 1, 1, 1, 0, 0]
    # every default rule (six leaves of the chain + the 256^2 kernel) under the default knobs, and the K % 128 != 0 fall-through
    # of the forced two-K-group forms 3, 4, 6 (the answer then differs from the form asked for)
    assert len({tuple(out(r, "nt")[:4]) for r in nt if r[13:19] == default}) == 8
    for form, kg_form in ((3, (128, 128, 2, 2)), (4, (128, 64, 2, 2)), (6, (128, 64, 3, 2))):
        asked = [r for r in nt if r[17] == form and r[1] > 64]
        assert any(tuple(out(r, "nt")[:4]) == kg_form for r in asked) and any(r[3] % 128 and out(r, "nt")[3] == 1 for r in asked)
    assert any(r[18] == 3 and tuple(out(r, "nt")[:4]) == (128, 128, 2, 2) for r in nt) and any(r[18] == 3 and out(r, "nt")[3] == 1 for r in nt)
    # the 256^2 rule: refused by the epilogue, by the knob, by the grid size; taken at a lowered min_tiles; forced
    big = [r for r in nt if r[1:4] == [4096, 2048, 2048] and r[13:19] == default]
    assert {(r[4], r[12], out(r, "nt")[0]) for r in big} >= {(1, 192, 128), (1, 128, 256), (0, 128, 128)}
    assert any(r[13] == 0 and r[1:4] == [8192, 2048, 2048] and out(r, "nt")[0] == 128 for r in nt)
    assert any(r[13] == 2 and r[1:4] == [2048, 2048, 2048] and out(r, "nt")[0] == 256 for r in nt)
    # tn128_split: both sites, the gate of the single launch (tiles >= target -> no split), each clamp binding, both split rules
    tn = by["tn128"]
    for single in (0, 1):
        rs = [r for r in tn if r[4] == single]
        assert len({out(r, "tn128")[0] for r in rs}) >= 12                                   # many different split factors
        assert any(out(r, "tn128")[0] == 32 for r in rs)                                      # the cap of 32 splits
        assert any(out(r, "tn128")[0] == r[3] and 0 < r[3] < 32 for r in rs)                  # slab capacity binds
        assert any(out(r, "tn128")[0] == r[2] and r[2] < 32 and r[3] == 1000 for r in rs)     # K-tile count binds
        assert any(r[6] == 0 and out(r, "tn128")[0] > 1 for r in rs)                          # tn_split_model 0
    assert any(r[4] == 1 and r[1] >= 512 and r[3] == 1000 and r[2] == 128 and out(r, "tn128")[0] == 1 for r in tn)
    assert any(r[4] == 0 and r[1] == 17 and r[2] == 128 and out(r, "tn128")[0] > 1 for r in tn)
    assert any(r[4] == 1 and r[1] == 16 and r[5] == 512 and r[6] == 0 and out(r, "tn128")[0] == 16 for r in tn)   # target 512 -> 256 at <= 16 tiles
    # the grouped launches of one bench.py train step (SmdEngine::flush_grouped_wgrads; grids of profiles/gemm_plan_*_train_kernel_trace.txt):
    # FiLM generators 296 tiles x 1 split, out_proj + up 80 x 3, an encoder layer 36 x 7, layer 0 + in_proj 40 x 6 -- with their real slab capacity
    default_tn = [512, 1, 2, 0, 1, 0]
    for tiles, kt, cap, nsplit in ((296, 4, 3, 1), (80, 128, 13, 3), (36, 128, 30, 7), (40, 128, 27, 6)):
        assert [out(r, "tn128")[0] for r in tn if r[1:5] == [tiles, kt, cap, 0] and r[5:11] == default_tn] == [nsplit]
    # tn128_mode: the four kernel variants and the three pad rules
    assert {tuple(out(r, "tn128")[2:4]) for r in tn} == {(4, 8), (4, 4), (2, 4), (2, 8)}
    assert {out(r, "tn128")[4] for r in tn} >= {0, 160 * 1024 - 4 * 32768, 96 * 1024 - 2 * 32768, 160 * 1024 - 2 * 32768}
    assert any(r[7] == 0 and r[8] == 1 and tuple(out(r, "tn128")[2:4]) == (4, 8) for r in tn)       # gemm_tn_deep on long splits
    assert any(r[7] == 0 and r[8] == 1 and tuple(out(r, "tn128")[2:4]) == (2, 4) for r in tn)
    # tn256_plan: eligible with 1 .. 4 splits, and each way of not being eligible; the forced mode beyond 4 splits
    t256 = by["tn256"]
    assert {out(r, "tn256")[0] for r in t256 if r[5] == 1} == {0, 1, 2, 3, 4}
    assert any(r[5] == 2 and out(r, "tn256")[0] > 4 for r in t256) and all(out(r, "tn256") == [0, 0] for r in t256 if r[5] == 0)
    assert any(out(r, "tn256")[1] % 2 == 0 and out(r, "tn256")[1] * out(r, "tn256")[0] > (r[1] + 63) // 64 for r in t256 if out(r, "tn256")[0])
    multi = by["tn256_multi"]
    assert {out(r, "tn256_multi")[0] for r in multi} >= {1, 2, 4} and len({tuple(out(r, "tn256_multi")) for r in multi}) >= 12
