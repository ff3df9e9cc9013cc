"""host/hierarchy.hpp and the -J -H -O rules of host/options.hpp without a GPU, through tests/helpers/hierarchy_check.cpp built
with -fsanitize=address,undefined: the order and the taxonomy of nested family labels are tests/hierarchy_ref.py's byte for
byte, parse_taxonomy takes the taxonomy, and the command lines the issue names are refused."""
import os
import subprocess

import numpy as np
import pytest

import families_ref as fr
import hierarchy_ref as hr
import test_gpu_hierarchy as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("hierarchy_check")
    exe = str(d / "hierarchy_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "hierarchy_check.cpp"), "-lz"], check=True)

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], cwd=str(d), capture_output=True, timeout=120)
        assert r.returncode in (0, 1) and not r.stderr, r.stderr.decode()[-2000:]
        return r.returncode, r.stdout.decode().split("\n")
    run.dir = str(d)
    return run


def lay_out(tool, labels, name):
    labels = np.ascontiguousarray(labels, np.uint32)
    L, G = labels.shape
    paths = [os.path.join(tool.dir, name + ext) for ext in (".labels", ".order", ".tax")]
    labels.tofile(paths[0])
    status, lines = tool("layout", L, G, *paths)
    return status, lines, paths


@pytest.fixture(scope="module")
def planted():
    return {b: th.Nested(b) for b in (8, 16)}


SMALL = {
    # name: (labels, nodes, depth, the taxonomy where it is written out by hand)
    "singletons": ([np.arange(7)], 7, 1, None),
    "one_family": ([np.zeros(5)], 6, 2, b"0 4 L0.0\n0 0 g0\n1 1 g1\n2 2 g2\n3 3 g3\n4 4 g4\n"),
    "repeats": ([[0, 0, 0, 3, 3, 5], [0, 0, 0, 3, 3, 5], [0, 0, 2, 3, 4, 5]], 9, 3,
                b"0 2 L0.0\n0 1 L2.0\n0 0 g0\n1 1 g1\n2 2 g2\n3 4 L0.3\n3 3 g3\n4 4 g4\n5 5 g5\n"),
    "interleaved": ([[0, 1, 0, 1]], 6, 2, b"0 1 L0.0\n0 0 g0\n1 1 g2\n2 3 L0.1\n2 2 g1\n3 3 g3\n"),
}


def check_layout(tool, labels, name):
    labels = np.asarray(labels, np.int64)
    L, G = labels.shape
    status, lines, (_, order_path, tax_path) = lay_out(tool, labels, name)
    assert status == 0, lines
    order, nodes = hr.layout(labels)
    got_order, got_tax = open(order_path, "rb").read(), open(tax_path, "rb").read()
    assert got_order == hr.order_bytes(order)
    assert got_tax == hr.taxonomy_bytes(nodes)
    assert lines[0].encode() == hr.summary_line(labels, nodes)
    assert lines[1] == "parsed %d" % len(nodes)                                          # parse_taxonomy takes it, node for node
    assert [int(x) for x in lines[2].split()] == [d for *_, d in nodes]
    placed = [int(x) for x in got_order.split()]
    assert sorted(placed) == list(range(G))                                              # a permutation
    # the level-0 families, read off the order file as runs of one label, are -F's families as sets
    runs = {}
    for p, j in enumerate(placed):
        runs.setdefault(int(labels[0, j]), []).append(p)
    assert all(r == list(range(r[0], r[0] + len(r))) for r in runs.values())
    from_f = [frozenset(int(x) for x in block.split()) for block in fr.format_labels(labels[0]).split(b"\n\n")]
    assert {frozenset(placed[p] for p in r) for r in runs.values()} == set(from_f)
    return nodes, got_tax


@pytest.mark.parametrize("fp_bits", [8, 16])
def test_planted_collections_lay_out_as_the_reference_does(tool, planted, fp_bits):
    n = planted[fp_bits]
    nodes, _ = check_layout(tool, n.want, "planted%d" % fp_bits)
    names = [name for _, _, name, _ in nodes]
    assert sum(name.startswith("g") for name in names) == n.G
    a0 = min(n.c.species_a)
    assert any(name.endswith(".%d" % a0) for name in names)                              # species A has a node
    if fp_bits == 16:
        assert not any(name.startswith("L1.") for name in names)                         # levels 0 and 1 repeat: one node, named L0
    else:
        assert nodes[0][:3] == (0, n.G - 1, "L0.0") and max(d for *_, d in nodes) >= 2


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_layouts(tool, name):
    labels, n_nodes, depth, tax = SMALL[name]
    nodes, got_tax = check_layout(tool, labels, name)
    assert len(nodes) == n_nodes and max(d for *_, d in nodes) + 1 == depth
    if tax is not None:
        assert got_tax == tax


def test_layouts_that_are_refused(tool):
    status, lines, _ = lay_out(tool, [[0, 1, 2], [0, 0, 2]], "no_nest")
    assert status == 1 and lines[0].startswith("refused: level 1") and "do not nest" in lines[0]
    status, lines, _ = lay_out(tool, [[1, 1]], "above")
    assert status == 1 and lines[0].startswith("refused: level 0") and "not the smallest id" in lines[0]
    status, lines, _ = lay_out(tool, [[0, 0, 2], [0, 1, 1]], "above_deeper")
    assert status == 1 and lines[0].startswith("refused: level 1")


def test_the_levels_of_J(tool):
    assert tool("levels", "10", 100) == (0, ["10 100", ""])
    assert tool("levels", "10:5.5,300:5.5", 100) == (0, ["10 5.5", "300 5.5", ""])
    assert tool("levels", "10:0.25,10,4000000000:1319.5", 2.5) == (0, ["10 0.25", "10 2.5", "4000000000 1319.5", ""])
    assert tool("levels", ",".join(["10"] * 8), 1)[0] == 0
    status, lines = tool("levels", ",".join(["10"] * 9), 1)
    assert status == 1 and "at most 8" in lines[0]
    for arg, level in (("10,5", 1), ("10:7,20:3", 1), ("10,20,20:1", 2), ("10,,20", 1), ("", 0), ("10,", 1), ("abc", 0), ("10:x", 0), ("1e3", 0),
                       ("-5", 0), ("10:5.", 0), ("10:.5", 0), ("10:-1", 0), ("5 ", 0), ("10:1:2", 0), ("99999999999", 0), ("10;20", 0)):
        status, lines = tool("levels", arg, 2)
        assert status == 1 and lines[0].startswith("refused: -J: level %d" % level), (arg, lines)


def test_the_three_flags_go_together_on_one_gpu(tool):
    I, J, H, O = ["-i", "none.idx"], ["-J", "10,300:250.5"], ["-H", "t.txt"], ["-O", "o.txt"]

    def refusal(args, devices=1, rank_mode=0, world=1):
        return tool("refusal", devices, rank_mode, 0, world, "miekki", *args)
    assert refusal([*I, *J, *H, *O, "-F", "f.txt", "-R", "r.txt", "-d", "d.idx"]) == (0, ["", "10 100", "300 250.5", ""])
    assert refusal(["-l", "g.lst", *J, *H, *O, "-s", "30"]) == (0, ["", "10 15", "300 250.5", ""])
    for args, word in (([*I, *J], "needs -H"), ([*I, *J, *H], "needs -O"), ([*I, *J, *O], "needs -H"), ([*I, *H], "need -J"), ([*I, *O], "need -J"),
                       ([*I, *H, *O], "need -J")):
        status, lines = refusal(args)
        assert status == 1 and word in lines[0], (args, lines)
    status, lines = refusal([*I, "-J", "10,5", *H, *O])
    assert status == 1 and lines[0].startswith("-J: level 1")
    status, lines = refusal([*I, *J, *H, *O], devices=2)
    assert status == 1 and "several GPUs" in lines[0] and "-J" in lines[0] and "MIEKKI_DEVICES" in lines[0]
    status, lines = refusal([*I, *J, *H, *O], rank_mode=1, world=2)
    assert status == 1 and "one process per GPU" in lines[0] and "-J" in lines[0]
    assert refusal([*I, "-F", "f.txt"], devices=2)[0] == 0                               # (-F alone is what it was)
