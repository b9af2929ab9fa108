"""tools/measure_common.py: the one runner of child processes, the kernel statistics, and the presets of the tools built on it.
Host only: the stand-in children are tiny scripts that import neither torch nor the package."""
import glob
import importlib.util
import inspect
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
PARENT_LINES = 3265                              # tools/measure_*.py together, before the shared module


def _load(name):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)                # a tool finds measure_common beside itself, as when it is run as a script
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mc():
    return _load("measure_common")


# A child that touches <dir>/<name>.marker, then does what its job says: exit with a status, stay silent, sleep, or pass.
CHILD = """import json, os, sys, time
job = json.loads(sys.argv[sys.argv.index("--child") + 1])
open(os.path.join(job["dir"], job["name"] + ".marker"), "w").close()
if "exit" in job:
    sys.exit(job["exit"])
if job.get("sleep"):
    time.sleep(job["sleep"])
if not job.get("silent"):
    print("some output before the result")
    print("RESULT " + json.dumps({"name": job["name"], "value": job.get("value", 0)}), flush=True)
"""


@pytest.fixture
def child(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    return str(script)


def _jobs(tmp_path, *extra):
    return [dict(dir=str(tmp_path), name="job%d" % (i + 1), value=10 * (i + 1), **e) for i, e in enumerate(extra)]


def _marker(tmp_path, i):
    return os.path.exists(os.path.join(str(tmp_path), "job%d.marker" % i))


@pytest.mark.parametrize("status", [1, 134, 139])
def test_first_failure_ends_the_run(mc, child, tmp_path, status):
    jobs = _jobs(tmp_path, {}, {"exit": status}, {})
    out = {"runs": []}
    assert mc.run_children(child, jobs, 20, out) is False
    assert [r["name"] for r in out["runs"]] == ["job1"]
    assert out["failed"] == {"job": jobs[1], "exit": status}
    assert _marker(tmp_path, 1) and _marker(tmp_path, 2) and not _marker(tmp_path, 3)


def test_no_result_line_is_a_failure(mc, child, tmp_path):
    jobs = _jobs(tmp_path, {"silent": True}, {})
    out = {"runs": []}
    assert mc.run_children(child, jobs, 20, out) is False
    assert out["runs"] == [] and out["failed"] == {"job": jobs[0], "exit": 0}
    assert _marker(tmp_path, 1) and not _marker(tmp_path, 2)


def test_time_limit_is_the_runners(mc, child, tmp_path):
    jobs = _jobs(tmp_path, {"sleep": 60}, {})
    out = {"runs": []}
    t0 = time.time()
    assert mc.run_children(child, jobs, 1, out) is False
    assert time.time() - t0 < 5.0
    assert out["failed"] == {"job": jobs[0], "exit": 124} and out["runs"] == []
    assert not _marker(tmp_path, 2)


def test_output_file_after_every_child(mc, child, tmp_path):
    path = tmp_path / "not" / "there" / "yet" / "out.json"
    seen = []

    def look(out, job, row):                     # the file already holds every row before this one
        seen.append(len(json.loads(path.read_text())["runs"]))

    jobs = _jobs(tmp_path, {}, {"exit": 1}, {})
    assert not mc.run_children(child, jobs, 20, {"tool": "t", "runs": []}, str(path), after_each=look)
    got = json.loads(path.read_text())
    assert got["tool"] == "t" and got["failed"] == {"job": jobs[1], "exit": 1}
    assert [r["name"] for r in got["runs"]] == ["job1"] and "child_wall_s" in got["runs"][0]
    seen.clear()
    assert mc.run_children(child, _jobs(tmp_path, {}, {}, {}), 20, {"tool": "t", "runs": []}, str(path), after_each=look)
    got = json.loads(path.read_text())
    assert [r["name"] for r in got["runs"]] == ["job1", "job2", "job3"] and "failed" not in got
    assert all("child_wall_s" in r for r in got["runs"])
    assert seen == [0, 1, 2]


def test_after_each(mc, child, tmp_path):
    calls = []

    def summarise(out, job, row):
        calls.append((job["name"], row["value"]))
        out["summary"] = {"sum": sum(r["value"] for r in out["runs"]), "last": job["name"]}

    out = {"runs": []}
    assert not mc.run_children(child, _jobs(tmp_path, {}, {}, {"exit": 1}, {}), 20, out, after_each=summarise)
    assert calls == [("job1", 10), ("job2", 20)]
    assert out["summary"] == {"sum": 30, "last": "job2"}


def test_argv_and_cwd_reach_the_child(mc, tmp_path):
    script = tmp_path / "where.py"
    script.write_text('import json, os, sys\nprint("RESULT " + json.dumps({"argv": sys.argv[1:3], "cwd": os.getcwd()}))\n')
    other = tmp_path / "other"
    other.mkdir()
    out = {"runs": []}
    assert mc.run_children(str(script), [{"part": "games"}], 20, out, argv=lambda job: [job["part"]], cwd=lambda job: str(other))
    assert out["runs"][0]["argv"] == ["games", "--child"] and os.path.samefile(out["runs"][0]["cwd"], str(other))


def test_emit_result_is_what_the_runner_reads(mc, tmp_path):
    script = tmp_path / "emit.py"
    script.write_text("import sys\nsys.path.insert(0, %r)\nimport measure_common\nmeasure_common.emit_result({'a': [1, 2]})\n" % TOOLS)
    out = {"runs": []}
    assert mc.run_children(str(script), [{}], 20, out)
    assert out["runs"][0]["a"] == [1, 2]


def _stats_csv(path, rows):
    with open(path, "w") as f:
        f.write('"Name","Calls","TotalDurationNs"\n')
        for name, calls, total in rows:
            f.write('"%s",%d,%d\n' % (name, calls, total))
    return str(path)


def test_kernel_statistics(mc, tmp_path):
    p = _stats_csv(tmp_path / "a_kernel_stats.csv", [("void k_select<0, false>(XqEngine)", 300, 3_000_000),
                                                     ("void k_select<2, true>(XqEngine)", 100, 3_000_000),
                                                     ("k_select_multi(XqEngine)", 1000, 900_000_000),
                                                     ("k_flush_records(XqEngine)", 10, 55_000)])
    assert mc.kernel_mean_us(p, "k_select", ("k_select_multi",)) == 15.0            # 6 000 000 ns / 400 calls
    assert mc.kernel_mean_us(p, "k_flush_records") == 5.5
    assert mc.kernel_mean_us(p, "k_reroot") is None
    assert mc.group([2.0, None, 3.5]) == {"runs": [2.0, 3.5], "min": 2.0, "max": 3.5, "spread": 1.5, "mean": 2.75}
    assert mc.group([1.0, 1.2346])["spread"] == 0.235 and mc.group([1.0, 1.2346])["mean"] == 1.117   # rounded to 3 places
    assert mc.group([]) is None and mc.group([None]) is None


def test_spread_groups(mc, tmp_path):
    def run(name, us):                           # one k_select instance at `us` microseconds per launch
        return _stats_csv(tmp_path / (name + "_kernel_stats.csv"), [("k_select<0>", 10, int(us * 10_000)), ("k_flush_records", 1, 2000)])

    parent = "parent=%s,%s" % (run("p1", 10.0), run("p2", 12.0))
    kernels = {"groups": ("k_select", ("k_select_multi",))}
    inside = mc.spread_groups([parent, "on=%s,%s" % (run("a1", 10.5), run("a2", 11.5))], kernels)
    assert inside["groups"]["parent"] == {"runs": [10.0, 12.0], "min": 10.0, "max": 12.0, "spread": 2.0, "mean": 11.0}
    assert inside["groups"]["on"]["mean"] == 11.0 and inside["on_within_parent_spread"] is True
    outside = mc.spread_groups([parent, "on=%s,%s" % (run("b1", 12.5), run("b2", 13.5))], kernels)
    assert outside["on_within_parent_spread"] is False
    assert "on_within_parent_spread" not in mc.spread_groups([parent], kernels)
    two = mc.spread_groups([parent, "off=%s" % run("c1", 11.0)], {"k_select": ("k_select", ()), "k_flush_records": ("k_flush_records", ())},
                           kinds=("off", "on"))
    assert two["off_within_parent_spread"] is True and "on_within_parent_spread" not in two
    assert two["k_flush_records"]["off"]["runs"] == [2.0]


TOOLS_WITH_TABLES = ("arena", "eval_cache", "eval_mirror", "forced_playouts", "game_records", "gumbel", "merge_duplicates",
                     "perpetual_check", "playout_cap", "policy_surprise", "root_stats", "solver", "tree_reuse")


def test_presets_did_not_move(mc):
    """tests/golden/tool_presets.json holds every tool's tables as they stood before the tools shared a module."""
    with open(os.path.join(ROOT, "tests", "golden", "tool_presets.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted("measure_" + t for t in TOOLS_WITH_TABLES)
    assert sum("PRESETS" in v for v in golden.values()) == 11
    assert inspect.signature(mc.make_net).parameters["gain"].default == 8.0
    for name, tables in golden.items():
        tool = _load(name)
        for key, want in tables.items():
            if key in ("GAINS", "PEAKED_GAIN") and not hasattr(tool, key):
                # a tool that no longer names its gain takes the shared table (make_net's default is its "peaked" entry)
                have = mc.GAINS if key == "GAINS" else mc.GAINS["peaked"]
            else:
                have = getattr(tool, key)
            assert json.loads(json.dumps(have)) == want, (name, key)


def test_import_weight():
    code = ("import sys; sys.path.insert(0, %r); import measure_common; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('torch', 'xiangqi_alphazero_amd', 'numpy')]; "
            "print(bad); sys.exit(1 if bad else 0)" % TOOLS)
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_one_copy():
    texts = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(TOOLS, "*.py"))}
    for needle in ('"timeout", "-k"', 'startswith("RESULT ")', "slots=1024, games=1024, sims=400"):
        assert [name for name, text in texts.items() if needle in text] == ["measure_common.py"], needle
    lines = sum(text.count("\n") for name, text in texts.items() if name.startswith("measure_"))
    assert lines < PARENT_LINES
