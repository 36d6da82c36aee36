"""The committed hand-scheduled attention loops (csrc/attn_x3_loop.inc, csrc/attn_hq2_loop.inc) are what their generators under
tools/gen/ write, byte for byte: the "GENERATED, do not edit" headers hold.  CPU only."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen")
CSRC = os.path.join(ROOT, "beat_this_amd", "csrc")


def run_gen(script, *args):
    return subprocess.run([sys.executable, os.path.join(GEN, script), *args], capture_output=True, text=True)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_generated_loops(tmp_path):
    for script, inc in (("attn_x3_loop.py", "attn_x3_loop.inc"), ("attn_hq2_loop.py", "attn_hq2_loop.inc")):
        out = tmp_path / inc
        r = run_gen(script, "-o", str(out))
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == read(os.path.join(CSRC, inc)), \
            f"{inc} differs from the output of tools/gen/{script}: regenerate it, do not edit it"
    # the committed x3 loop holds the statements that are built and nothing else
    committed = read(os.path.join(CSRC, "attn_x3_loop.inc"))
    assert b"#if" not in committed and b"_ABL" not in committed
    # an ablated listing (--abl) is never written into the sources: not under a new name, not over the committed file through
    # a path with .. in it, not by default
    before = sorted(os.listdir(CSRC))
    for path in (os.path.join(CSRC, "attn_x3_abl1.inc"), os.path.join(CSRC, "..", "csrc", "attn_x3_loop.inc"), None):
        r = run_gen("attn_x3_loop.py", "--abl", "1", *(["-o", path] if path else []))
        assert r.returncode != 0 and "csrc" in r.stderr, (path, r.stderr)
    assert sorted(os.listdir(CSRC)) == before and read(os.path.join(CSRC, "attn_x3_loop.inc")) == committed
    # elsewhere it is written: 1 = the loop without its softmax VALU instructions
    out = tmp_path / "abl1.inc"
    r = run_gen("attn_x3_loop.py", "--abl", "1", "-o", str(out))
    assert r.returncode == 0, r.stderr
    text = out.read_text()
    assert "#define ATTN_X3Q2_ASM" in text and "v_mfma" in text and "v_exp_f32" not in text
