"""llama_box_amd/csrc/options.h without a GPU: tests/options_probe.cpp, a plain C++ program over that header, compiled once and run as a child process.

CONTRACT below is what hosts rely on: every per-backend option's set_option key, storage type, default and environment variable, written down from
struct options and init_backend as they stood before the options became one table.  It is not regenerated from the header: an option added later is
added here on purpose."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "llama_box_amd", "csrc")

# key, type, default, has an environment variable (GGML_MI355X_<KEY>), a write stores value != 0
CONTRACT = [
    ("graphs", "bool", 1, True, True),
    ("fusion", "bool", 1, True, True),
    ("prologue", "bool", 1, True, True),
    ("qkv", "bool", 1, True, True),
    ("mmvq_max_cols", "int", 2, True, False),
    ("mmq_min_cols", "int", 3, True, False),
    ("mmq_i8", "bool", 1, True, True),
    ("mm_merge", "bool", 1, True, True),
    ("ss_partials", "bool", 1, True, True),
    ("fa_self_merge", "bool", 0, True, True),
    ("attn_nf", "bool", 1, True, True),
    ("softmax_mm", "bool", 1, True, True),
    ("skinny_rope", "bool", 1, True, True),
    ("skinny_mix", "bool", 1, True, True),
    ("mmq_skinny", "bool", 1, True, True),
    ("mmq_bn", "int", 0, True, False),
    ("bf16_form", "int", -1, True, False),
    ("bf16_mmv_max_cols", "int", 8, True, False),
    ("bf16_nt", "int", 1, True, True),
    ("bf16_preround", "int", 1, True, True),
    ("fa_splits", "int", 0, True, False),
    ("fa_wo", "bool", 0, True, True),
    ("small_uploads", "bool", 1, True, True),
    ("small_downloads", "bool", 1, True, True),
    ("timing", "bool", 0, False, True),
    ("decode_copy_headroom_gib", "int", 2, False, False),
    ("decode_copy", "bool", 1, True, True),
    ("exec_update", "int", 1, True, False),
    ("shadow_capture", "int", 1, True, False),
    ("q80_min_cols", "int", 33, True, False),
]
DEFAULTS = {k: d for k, _, d, _, _ in CONTRACT}


def env_name(key):
    return "GGML_MI355X_" + key.upper()


def non_default(default, flag):
    """What the tests write: the other state of a flag, default + 7 for a number."""
    return (0 if default else 1) if flag else default + 7


def stored(value, flag):
    return int(value != 0) if flag else value


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("options_probe") / "options_probe")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", CSRC, os.path.join(REPO, "tests", "options_probe.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr  # (a warning fails it too)

    def run(*args, env=None):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("GGML_MI355X_")}
        clean.update(env or {})
        p = subprocess.run([exe, *args], capture_output=True, text=True, env=clean)
        assert p.returncode == 0, (args, p.returncode, p.stdout, p.stderr)
        return p.stdout.splitlines()

    return run


def test_every_option_keeps_its_key_type_default_and_variable(probe):
    want = [f"{k} {t} {d} {env_name(k) if has_env else '-'}" for k, t, d, has_env, _ in CONTRACT]
    assert sorted(probe("rows")) == sorted(want)


def fields(lines):
    return {k: int(v) for k, v in (ln.split() for ln in lines)}


def test_nothing_set_gives_the_defaults(probe):
    assert fields(probe("env")) == DEFAULTS


def test_environment_reaches_every_option_that_has_a_variable(probe):
    env, want = {}, {}
    for k, t, d, has_env, flag in CONTRACT:
        v = non_default(d, flag)
        env[env_name(k)] = str(v)
        want[k] = stored(v, flag) if has_env else d
    env["GGML_MI355X_TIMING"] = "1"  # (no such variables: they must change nothing)
    env["GGML_MI355X_DECODE_COPY_HEADROOM_GIB"] = "9"
    got = fields(probe("env", env=env))
    assert got == want
    assert got["bf16_nt"] == 0 and got["bf16_preround"] == 0 and got["timing"] == 0 and got["decode_copy_headroom_gib"] == 2
    # the two flags kept in an int: 0 above was read, and 5 is stored as 1
    env.update({"GGML_MI355X_BF16_NT": "5", "GGML_MI355X_BF16_PREROUND": "5"})
    assert fields(probe("env", env=env)) == {**want, "bf16_nt": 1, "bf16_preround": 1}


def parse_set(line):
    rc, eq, *kv = line.split()
    return int(rc.split("=")[1]), int(eq.split("=")[1]), {k: int(v) for k, v in (x.split("=") for x in kv)}


@pytest.mark.parametrize("key,typ,default,has_env,flag", CONTRACT, ids=[c[0] for c in CONTRACT])
def test_set_changes_that_field_and_equality_sees_it(probe, key, typ, default, has_env, flag):
    v = non_default(default, flag)
    there, back = (parse_set(ln) for ln in probe("set", f"{key}={v}", f"{key}={default}"))
    assert there == (1, 0, {**DEFAULTS, key: stored(v, flag)})  # accepted; only this field differs; no longer equal to default options
    assert back == (1, 1, DEFAULTS)
    if flag:
        assert parse_set(probe("set", f"{key}=5")[0])[2][key] == 1  # value != 0 is what is stored


def test_unknown_and_empty_keys_are_refused(probe):
    for ln in probe("set", "nope=1", "=1", "GRAPHS=0", "graphs =0", "tp_p2p=1", "staged_upload=1"):
        assert parse_set(ln) == (0, 1, DEFAULTS)


# counters hosts and tests read through get_stat, as they spell them (the whole list as a backend answers it: tests/test_gpu_option_keys.py)
STAT_KEYS = ["graph_launches", "kernel_launches", "fused_nodes", "nf_mma_chains", "nf_list_chains", "fa_form", "fa_list_launches", "skinny_launches", "mmid_launches"]


def test_stat_keys_are_in_the_table_and_start_at_zero(probe):
    got = fields(probe("stats"))
    assert all(v == 0 for v in got.values()), got  # (-1: stats_find does not return the counter of that name)
    for key in STAT_KEYS:
        assert key in got, key


def test_env_helpers_mean_what_the_spelled_out_reads_meant(probe):
    # value: env_flag(name, true), env_flag(name, false), env_int(name, 7), env_present(name) — and "same" = equal to the four getenv idioms the probe spells out
    want = {"unset": (1, 0, 7, 0), "empty": (0, 0, 0, 1), "0": (0, 0, 0, 1), "1": (1, 1, 1, 1), "2": (1, 1, 2, 1), "x": (0, 0, 0, 1)}
    lines = probe("helpers")
    assert len(lines) == len(want)
    for ln in lines:
        m = re.fullmatch(r"(\S+) flag_true=(\d) flag_false=(\d) int7=(-?\d+) present=(\d) (\S+)", ln)
        assert m, ln
        assert tuple(int(x) for x in m.groups()[1:5]) == want[m.group(1)] and m.group(6) == "same", ln


def test_every_option_is_documented(probe):
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    sec = text[text.index("## 4b."):text.index("## 4c.")]
    for row in probe("rows"):  # (the header's rows, so that an option added there without a line in the document fails here)
        k, _, _, env = row.split()
        name = k if env == "-" else env
        assert re.search(r"`" + re.escape(name) + r"`", sec), f"{name} has no row in INTEGRATION.md 4b"
