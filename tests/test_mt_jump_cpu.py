"""CPU-only: jump-ahead for MT19937 (host/mt_jump.hpp + csrc/fm_mt_jump_table.hpp, written by tools/mt_jump_table.py).  The C++ driver
tests/cpp/test_mt_jump.cpp checks jump(n) against stepping n words for n around the block and table edges and 10^7 + 3, composition
(far jumps included), the published MT19937 known answers behind a jump of 0, and the 2^44 limit; the table's --check recomputes the
minimal polynomial and every t^(2^j) mod φ and compares with the committed header."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd")


def test_jump_equals_stepping_and_composes(tmp_path):
    exe = str(tmp_path / "test_mt_jump")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mt_jump.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK"


def test_table_check_is_clean():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mt_jump_table.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr


def test_table_check_sees_drift(tmp_path):
    """--check compares with the header beside the tool: a copy of the tool next to a header with one flipped bit must exit 1."""
    tools = tmp_path / "tools"; csrc = tmp_path / "finmath-lib-cuda-extensions_amd" / "csrc"
    tools.mkdir(); csrc.mkdir(parents=True)
    (tools / "mt_jump_table.py").write_text(open(os.path.join(ROOT, "tools", "mt_jump_table.py"), encoding="utf-8").read(), encoding="utf-8")
    text = open(os.path.join(PKG, "csrc", "fm_mt_jump_table.hpp"), encoding="utf-8").read()
    (csrc / "fm_mt_jump_table.hpp").write_text(text.replace("{ // 2^0\n    0x2,", "{ // 2^0\n    0x3,", 1), encoding="utf-8")
    assert text.count("{ // 2^0\n    0x2,") == 1
    out = subprocess.run([sys.executable, str(tools / "mt_jump_table.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 1 and "DRIFT" in out.stdout


def test_table_shape():
    text = open(os.path.join(PKG, "csrc", "fm_mt_jump_table.hpp"), encoding="utf-8").read()
    assert "FM_MT_JUMP_TABLE[44][624]" in text and text.count("{ // 2^") == 44
