"""What the command-line tests share: the path of the built `miekki` binary, one run of it, and the read files and the
output lines most of them use."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "miekki_amd", "miekki")


def cli(args, cwd, devices="0", env=None, ok=True):
    e = dict(os.environ, MIEKKI_DEVICES=devices)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([CLI, *args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=e)
    if ok:
        assert r.returncode == 0, r.stdout.decode(errors="replace")
    return r


def records(reads):
    return b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))


def line_of(out, head):
    """the lines that `head` starts, behind the reader's progress marks where it is the first after them"""
    return [l.lstrip(b"-") for l in out.split(b"\n") if l.lstrip(b"-").startswith(head)]
