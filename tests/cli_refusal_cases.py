"""The command lines that `miekki` refuses before it makes a context, as a table: at least one per rule of
host/options.hpp's refusal(), in the rules' order, and a few that break two rules, whose first message is the one to come.
The expected first stdout line and exit status of each, tests/golden/cli_refusals.json, were recorded from the binary of the
commit before the rules became a table:
    python tests/cli_refusal_cases.py <binary>  >  tests/golden/cli_refusals.json
MIEKKI_DEVICES is always set, so no device is counted, and no case gets as far as opening one.  ACCEPTED: command lines
that no rule refuses (they are not run through the binary: it would go on to the device)."""
import json
import os
import subprocess
import sys
import tempfile

RANKED = {"MIEKKI_WORLD": "2", "MIEKKI_RANK": "0"}
SINKS = "PpyCWDG"
# what lets a sink flag through the rules before the one a case is after: -p goes with -L, -y with -T
SINK_ARGS = {"P": ["-P", "o.txt"], "p": ["-p", "o.txt", "-L", "good.clades"], "y": ["-y", "o.txt", "-T", "good.tax"],
             "C": ["-C", "o.txt"], "W": ["-W", "o.txt"], "D": ["-D", "o.txt"], "G": ["-G", "o.txt"]}
I = ["-i", "none.idx"]
A = ["-a", "r.fa"]

FILES = {
    "r.fa": b">r0\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n",
    "r.fq": b"@r0\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n",
    "genomes.lst": b"r.fa\n",
    "samples.lst": b"r.fq\nr.fq\n",
    "samples_fa.lst": b"r.fq\nr.fa\n",
    "samples_gone.lst": b"r.fq\ngone.fq\n",
    "empty.lst": b"\n",
    "good.keep": b"1\n0\n",
    "word.keep": b"0\nfirst\n",
    "twice.keep": b"2\n\n2\n",
    "empty.keep": b"\n\n",
    "good.clades": b"0\n1\n\n2\n",
    "word.clades": b"0\nx\n",
    "order.clades": b"3\n1\n",
    "empty.clades": b"\n",
    "good.tax": b"0 3 root\n0 1 left\n2 3 right\n",
    "word.tax": b"0 three\n",
    "back.tax": b"3 1\n",
    "order.tax": b"2 3 a\n0 1 b\n",
}


def case(name, args, devices="0", env=None):
    return {"name": name, "args": args, "devices": devices, "env": env or {}}


CASES = [
    case("M_needs_i", ["-M", "b.idx", *A]),
    case("M_with_l", ["-M", "b.idx", "-l", "genomes.lst"]),
    case("2_needs_a", [*I, "-2", "r.fa"]),
    case("2_with_e", [*I, *A, "-2", "r.fa", "-e"]),
    case("2_with_S", [*I, *A, "-2", "r.fa", "-S", "samples.lst", "-c", "c.txt"]),
    case("2_unreadable", [*I, *A, "-2", "gone.fa"]),
    *[case(f"{s}_needs_a", [*I, *SINK_ARGS[s]]) for s in SINKS],
    *[case(f"{s}_with_{x[0][1]}", [*I, *A, *SINK_ARGS[s], *x]) for s, x in zip(SINKS, (["-e"], ["-A", "genomes.lst"], ["-X"], ["-e"], ["-A", "genomes.lst"], ["-X"], ["-e"]))],
    *[case(f"{s}_with_n", [*I, *A, *SINK_ARGS[s], "-n", "5"]) for s in SINKS],
    case("S_needs_c", [*I, "-S", "samples.lst"]),
    case("c_needs_S", [*I, "-c", "c.txt"]),
    case("S_with_a", [*I, *A, "-S", "samples.lst", "-c", "c.txt"]),
    case("S_with_X", [*I, "-X", "-S", "samples.lst", "-c", "c.txt"]),
    case("S_with_n", [*I, "-S", "samples.lst", "-c", "c.txt", "-n", "5"]),
    case("S_unreadable", [*I, "-S", "gone.lst", "-c", "c.txt"]),
    case("S_names_none", [*I, "-S", "empty.lst", "-c", "c.txt"]),
    case("S_sample_gone", [*I, "-S", "samples_gone.lst", "-c", "c.txt"]),
    case("p_needs_L", [*I, *A, "-p", "o.txt"]),
    case("L_needs_p", [*I, *A, "-L", "good.clades"]),
    case("y_needs_T", [*I, *A, "-y", "o.txt"]),
    case("T_needs_y", [*I, *A, "-T", "good.tax"]),
    case("Y_needs_T", [*I, *A, "-Y", "n.txt"]),
    case("m_needs_T", [*I, *A, "-m", "50"]),
    case("m_beyond", [*I, *A, *SINK_ARGS["y"], "-m", "101"]),
    case("m_word", [*I, *A, *SINK_ARGS["y"], "-m", "5x"]),
    case("g_needs_G", [*I, *A, "-g", "5"]),
    case("g_zero", [*I, *A, "-G", "o.txt", "-g", "0"]),
    case("n_negative", [*I, *A, "-n", "-1"]),
    case("n_beyond", [*I, *A, "-n", "4294967294"]),
    case("n_with_e", [*I, *A, "-n", "5", "-e"]),
    case("X_with_a", [*I, *A, "-X"]),
    case("X_with_e", [*I, "-X", "-e"]),
    case("rank_beyond_world", [*I, *A], env={"MIEKKI_WORLD": "2", "MIEKKI_RANK": "5"}),
    case("rank_from_launcher", [*I, *A, "-n", "5"], env={"WORLD_SIZE": "2", "RANK": "0"}),
    case("ranked_n", [*I, *A, "-n", "5"], env=RANKED),
    case("ranked_n_all", [*I, *A, "-n", "0"], env=RANKED),
    case("ranked_X", [*I, "-X"], env=RANKED),
    case("ranked_K", [*I, "-K", "good.keep"], env=RANKED),
    case("ranked_F", [*I, "-F", "f.txt"], env=RANKED),
    case("ranked_R", [*I, "-R", "f.txt"], env=RANKED),
    case("ranked_r", [*I, "-r", "f.txt"], env=RANKED),
    case("several_R", [*I, "-R", "f.txt"], devices="0,0"),
    case("several_r", [*I, "-r", "f.txt"], devices="0,0"),
    case("q_needs_a", [*I, "-q", "20"]),
    case("q_with_e", [*I, *A, "-q", "20", "-e"]),
    case("q_with_A", [*I, "-a", "r.fq", "-A", "genomes.lst", "-q", "20"]),
    case("q_beyond", [*I, "-a", "r.fq", "-q", "94"]),
    case("q_word", [*I, "-a", "r.fq", "-q", "2o"]),
    case("q_not_fastq", [*I, *A, "-q", "20"]),
    case("q_mates_not_fastq", [*I, "-a", "r.fq", "-2", "r.fa", "-q", "20"]),
    case("q_sample_not_fastq", [*I, "-S", "samples_fa.lst", "-c", "c.txt", "-q", "20"]),
    case("ranked_q", [*I, "-a", "r.fq", "-q", "20"], env=RANKED),
    case("several_q", [*I, "-a", "r.fq", "-q", "20"], devices="0,0"),
    case("ranked_2", [*I, *A, "-2", "r.fa"], env=RANKED),
    case("several_2", [*I, *A, "-2", "r.fa"], devices="0,0"),
    *[case(f"ranked_{s}", [*I, *A, *SINK_ARGS[s]], env=RANKED) for s in SINKS],
    *[case(f"several_{s}", [*I, *A, *SINK_ARGS[s]], devices="0,0") for s in SINKS],
    case("ranked_S", [*I, "-S", "samples.lst", "-c", "c.txt"], env=RANKED),
    case("several_S", [*I, "-S", "samples.lst", "-c", "c.txt"], devices="0,0"),
    case("ranked_M", [*I, "-M", "b.idx"], env=RANKED),
    case("several_M", [*I, "-M", "b.idx"], devices="0,0"),
    case("K_unreadable", [*I, "-K", "gone.keep"]),
    case("K_word", [*I, "-K", "word.keep"]),
    case("K_twice", [*I, "-K", "twice.keep"]),
    case("K_empty", [*I, "-K", "empty.keep"]),
    case("L_unreadable", [*I, *A, "-p", "o.txt", "-L", "gone.clades"]),
    case("L_word", [*I, *A, "-p", "o.txt", "-L", "word.clades"]),
    case("L_order", [*I, *A, "-p", "o.txt", "-L", "order.clades"]),
    case("L_empty", [*I, *A, "-p", "o.txt", "-L", "empty.clades"]),
    case("T_unreadable", [*I, *A, "-y", "o.txt", "-T", "gone.tax"]),
    case("T_word", [*I, *A, "-y", "o.txt", "-T", "word.tax"]),
    case("T_back", [*I, *A, "-y", "o.txt", "-T", "back.tax"]),
    case("T_order", [*I, *A, "-y", "o.txt", "-T", "order.tax"]),
    # two rules broken: the earlier one speaks
    case("first_M_then_2", ["-M", "b.idx", "-2", "r.fa"]),
    case("first_2_then_P", [*I, "-2", "r.fa", "-P", "o.txt"]),
    case("first_P_then_C", [*I, *A, "-C", "o.txt", "-P", "o.txt", "-n", "3"]),
    case("first_sink_then_S", [*I, "-P", "o.txt", "-S", "samples.lst"]),
    case("first_m_then_g", [*I, *A, *SINK_ARGS["y"], "-m", "200", "-g", "5"]),
    case("first_n_then_rank", [*I, *A, "-n", "-3"], env=RANKED),
    case("first_q_range_then_several", [*I, "-a", "r.fq", "-q", "99"], devices="0,0"),
    case("first_q_fastq_then_ranked", [*I, *A, "-q", "20"], env=RANKED),
    case("first_R_then_q", [*I, "-a", "r.fq", "-q", "99", "-R", "f.txt"], devices="0,0"),
    case("first_q_then_2", [*I, "-a", "r.fq", "-2", "r.fq", "-q", "20"], devices="0,0"),
    case("first_2_then_P_several", [*I, *A, "-2", "r.fa", "-P", "o.txt"], devices="0,0"),
    case("first_P_then_G_several", [*I, *A, "-G", "o.txt", "-P", "o.txt"], devices="0,0"),
    case("first_P_ranked_then_several", [*I, *A, "-P", "o.txt"], devices="0,0", env=RANKED),
    case("first_several_then_K_file", [*I, *A, "-P", "o.txt", "-K", "gone.keep"], devices="0,0"),
    case("first_K_then_L", [*I, *A, "-K", "word.keep", "-p", "o.txt", "-L", "word.clades"]),
    case("first_L_then_T", [*I, *A, "-p", "o.txt", "-L", "word.clades", "-y", "o.txt", "-T", "word.tax"]),
    # another rank than 0: silent from the rank rules on, heard before them
    case("rank1_before_silence", [*I, *A, "-n", "-1"], env={"MIEKKI_WORLD": "2", "MIEKKI_RANK": "1"}),
    case("rank1_silent", [*I, *A, "-n", "5"], env={"MIEKKI_WORLD": "2", "MIEKKI_RANK": "1"}),
    case("rank1_silent_file", [*I, "-K", "gone.keep"], env={"MIEKKI_WORLD": "2", "MIEKKI_RANK": "1"}),
]

ALL_SINKS = ["-P", "a.txt", "-p", "b.txt", "-L", "good.clades", "-y", "c.txt", "-T", "good.tax", "-Y", "d.txt", "-m", "50",
             "-C", "e.txt", "-W", "f.txt", "-D", "g.txt", "-G", "h.txt", "-g", "5"]
ACCEPTED = [
    case("build_and_query", ["-l", "genomes.lst", *A, "-o", "out.txt", "-h", "12", "-k", "21", "-s", "10", "-t", "2", "-f", "3", "-b", "20"]),
    case("load_and_query", [*I, *A, "-n", "0"]),
    case("exact", ["-l", "genomes.lst", *A, "-e"]),
    case("whole_files", [*I, "-A", "genomes.lst", "-n", "64"]),
    case("whole_files_exact", ["-l", "genomes.lst", "-A", "genomes.lst", "-e"]),
    case("index_queries", [*I, "-X", "-n", "3"]),
    case("dump", ["-l", "genomes.lst", "-d", "d.idx"]),
    case("keep_families_reps", [*I, "-K", "good.keep", "-F", "f.txt", "-R", "r.txt", "-r", "c.txt", "-d", "d.idx"]),
    case("join", [*I, "-M", "b.idx", "-M", "c.idx", "-X"]),
    case("pairs", [*I, *A, "-2", "r.fa", "-n", "3"]),
    case("quality", [*I, "-a", "r.fq", "-2", "r.fq", "-q", "20"]),
    case("panel", [*I, "-S", "samples.lst", "-c", "c.txt", "-q", "0"]),
    case("all_sinks", [*I, "-a", "r.fq", "-2", "r.fq", "-q", "93", *ALL_SINKS]),
    case("several_gpus", [*I, *A, "-K", "good.keep", "-F", "f.txt", "-n", "0"], devices="0,0"),
    case("ranked", ["-l", "genomes.lst", *A, "-e", "-d", "d.idx"], env=RANKED),
    case("ranked_rank1", ["-l", "genomes.lst", *A], env={"WORLD_SIZE": "2", "RANK": "1", "LOCAL_RANK": "1"}),
]


def write_files(d):
    for name, data in FILES.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)


def environment(c):
    e = dict(os.environ, MIEKKI_DEVICES=c["devices"])
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK", "MIEKKI_LOCAL_RANK"):
        e.pop(k, None)
    e.update(c["env"])
    return e


def where(c):
    """[devices, rank_mode, rank_id, rank_world] as the binary reads them from the case's environment"""
    env = c["env"]
    world = int(env.get("MIEKKI_WORLD", env.get("WORLD_SIZE", 1)))
    rank = int(env.get("MIEKKI_RANK", env.get("RANK", 0)))
    return [len(c["devices"].split(",")), int(world > 1 or "MIEKKI_WORLD" in env), rank, world]


def first_line_and_status(argv, c, cwd):
    r = subprocess.run(argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=environment(c))
    return {"line": r.stdout.decode(errors="replace").split("\n")[0], "status": r.returncode}


def record(binary):
    with tempfile.TemporaryDirectory() as d:
        write_files(d)
        return {c["name"]: first_line_and_status([os.path.abspath(binary), *c["args"]], c, d) for c in CASES}


if __name__ == "__main__":
    print(json.dumps(record(sys.argv[1]), indent=1, sort_keys=True))
