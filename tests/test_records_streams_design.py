"""The records streams of a trace (csrc/host/problem.c: trace_impl), without a GPU: problem.c's trace
path compiled against a RECORDING stub of the hrt_hip_* layer (tests/records_streams_stub.c) and the recorded call
sequence checked -- which stream every records kernel goes to, what it waited for, what the caller's stream waits for at
the end -- for 1, 2 and 3 streams; and that a trace which must not fork (a timer, HRT_OVERLAP=0, no patch masks, the
chain kernel) and HRT_OVERLAP=1 make exactly the calls the code made before there were several streams:
tests/golden/records_streams_parent_calls.json holds those, recorded with the same stub from the commit before
(`python -m tests.test_records_streams_design <that checkout>` wrote it).  The stub program is built a second time with
-fsanitize=address,undefined and run over every case."""
import json
import os
import re
import subprocess
import sys

import pytest

from tests.test_launch_plan_design import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "records_streams_parent_calls.json")
NB = (1, 2, 4, 5, 8)
STREAMS = (1, 2, 3)
T_PATCH, T_CHAIN = 234, 40   # a patch-table problem (65 .. 256 triangles); a table the chain kernel takes (<= 64)
# mode -> (environment, triangles, patch masks, timer)
PARENT_MODES = {
    "overlap1": ({"HRT_OVERLAP": "1"}, T_PATCH, 1, 0),
    "overlap0": ({"HRT_OVERLAP": "0"}, T_PATCH, 1, 0),
    "timer": ({}, T_PATCH, 1, 1),
    "nomask": ({}, T_PATCH, 0, 0),
    "chain": ({}, T_CHAIN, 0, 0),
}


def build_stub(tree, out, sanitize=False):
    """problem.c, tune.c and accel.c of `tree` + the recording stub as one host program (plain C, its own main)"""
    r = os.path.join(tree, "hermespy-rt_amd")
    cmd = ["cc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-ffunction-sections", "-fdata-sections", "-pthread",
           "-DHRT_BUILD", "-I", os.path.join(tree, "include"), "-I", os.path.join(r, "csrc"), "-I", os.path.join(r, "csrc", "host")]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    cmd += [os.path.join(REPO, "tests", "records_streams_stub.c")]
    cmd += [os.path.join(r, "csrc", "host", f) for f in ("problem.c", "tune.c", "accel.c")]
    subprocess.check_call(cmd + ["-lm", "-Wl,--gc-sections", "-o", out])
    return out


def run(exe, nb, tri=T_PATCH, masks=1, timer=0, traces=2, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("HRT_TUNE", "HRT_OVERLAP", "HRT_FUSE")}
    e.update(env or {})
    p = subprocess.run([exe, str(nb), str(tri), str(masks), str(timer), str(traces)], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout.splitlines()


def parent_cases(exe):
    return {"%s/%d" % (m, nb): run(exe, nb, tri, masks, timer, 2, env)
            for m, (env, tri, masks, timer) in PARENT_MODES.items() for nb in NB}


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return build_stub(REPO, str(tmp_path_factory.mktemp("streams") / "records_streams_stub"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def traces_of(lines):
    """the log split at its '-- ...' marks: [trace 0, trace 1, ..., destroy]"""
    parts = []
    for l in lines:
        if l.startswith("-- "):
            parts.append([])
        else:
            parts[-1].append(l)
    return parts


KERNEL = re.compile(r"^(fused|trace|image|shade|records|chain|sort) b0?=(\d+) on (\w+)$")


def check_trace(log, nb, A, created_before):
    """one trace's calls: every claim of the schedule, from the log alone"""
    made = [l for l in log if l.startswith("stream_create")]
    n_streams = min(A, nb)
    assert len(made) == (0 if created_before else n_streams), made
    where = {}                      # launch -> index of its records kernel
    last_main_kernel = {}           # launch -> index of its last kernel on the caller's stream
    recorded = {}                   # event -> (index, stream) of its LATEST record so far
    waited = {}                     # index of a wait -> (stream, event, index and stream of the record it sees)
    for i, l in enumerate(log):
        m = KERNEL.match(l)
        if m and m.group(1) == "records":
            where[int(m.group(2))] = i
        elif m:
            assert m.group(3) == "main", l
            last_main_kernel[int(m.group(2))] = i
        elif l.startswith("record "):
            _, ev, _, st = l.split()
            recorded[ev] = (i, st)
        elif l.startswith("wait "):
            _, ev, _, st = l.split()
            assert ev in recorded, l            # never a wait on an event that was not recorded in this trace
            waited[i] = (st, ev) + recorded[ev]
    assert sorted(where) == list(range(1, nb + 1))
    last_records_on = {}
    for b in range(1, nb + 1):
        i = where[b]
        st = "aux%d" % ((b - 1) % A)
        assert log[i] == "records b=%d on %s" % (b, st), log[i]
        # the stream's call before it: a wait on an event recorded on the caller's stream behind launch b - 1's last
        # kernel and in front of every kernel of launch b
        ops = [j for j in range(i) if log[j].endswith(" on " + st)]
        assert ops and ops[-1] in waited, (b, log[ops[-1]] if ops else None)
        w_st, _, r_i, r_st = waited[ops[-1]]
        assert (w_st, r_st) == (st, "main")
        assert last_main_kernel[b - 1] < r_i < ops[-1] < i
        assert not any(KERNEL.match(log[j]) and int(KERNEL.match(log[j]).group(2)) == b for j in range(r_i)), b
        last_records_on[st] = i
    assert sorted(last_records_on) == ["aux%d" % k for k in range(n_streams)]
    # the join: the caller's stream waits, behind everything else of the trace, on an event recorded on each used
    # stream after that stream's last records kernel
    joined = {}
    for i, (st, ev, r_i, r_st) in waited.items():
        if st == "main":
            assert r_st != "main" and r_i > last_records_on[r_st] and i > max(where.values()), log[i]
            assert not any(l.endswith(" on " + r_st) for l in log[r_i + 1:]), r_st   # nothing behind the record
            joined[r_st] = i
    assert sorted(joined) == sorted(last_records_on)
    assert all(i > max(last_main_kernel.values()) for i in joined.values())
    return made


@pytest.mark.parametrize("A", STREAMS)
@pytest.mark.parametrize("nb", NB)
def test_records_go_round_the_streams_fork_behind_their_launch_and_all_join(stub, nb, A):
    for prio in (1, 0):
        log = run(stub, nb, env={"HRT_TUNE": "aux_streams=%d,aux_prio=%d" % (A, prio)})
        t0, t1, destroy = traces_of(log)
        made = check_trace(t0, nb, A, created_before=False)
        assert all(l.startswith("stream_create %s " % ("lowest" if prio else "default")) for l in made), made
        # the second trace makes nothing, and its memset and launch 0 stand behind the joins of the first: the caller's
        # stream is in order, and the first trace's last calls on it are the waits on every used stream
        assert not any("create" in l for l in t1)
        check_trace(t1, nb, A, created_before=True)
        assert t0[-1].startswith("wait ") and t0[-1].endswith(" on main") and t1[1] == "memset 0 on main"
        n = min(A, nb)
        assert sorted(l for l in destroy if l.startswith("stream_destroy")) == ["stream_destroy aux%d" % k for k in range(n)]
        assert len([l for l in destroy if l.startswith("event_destroy")]) == 2 * n


def test_the_default_is_two_streams_at_the_lowest_priority(stub):
    assert run(stub, 5) == run(stub, 5, env={"HRT_TUNE": "aux_streams=2,aux_prio=1"})
    for bad in ("aux_streams=0", "aux_streams=4", "aux_prio=2", "aux_streams=10"):
        e = dict(os.environ, HRT_TUNE=bad)
        assert subprocess.run([stub, "2", str(T_PATCH), "1", "0", "1"], env=e, stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL).returncode == 4, bad


def _without_aux_objects(lines):
    """the calls that enqueue work: without the making and the freeing of records streams and their events"""
    return [l for l in lines if not re.match(r"^(stream_create|stream_destroy|event_create_sync|event_destroy ev\d)", l)]


@pytest.mark.parametrize("nb", NB)
def test_one_stream_at_the_default_priority_is_the_schedule_of_before(stub, golden, nb):
    """HRT_OVERLAP=1: call for call"""
    log = run(stub, nb, env={"HRT_OVERLAP": "1"})
    assert log == golden["overlap1/%d" % nb]
    assert [l for l in log if l.startswith("stream_create")] == ["stream_create default -> aux0"]
    # ... whatever HRT_TUNE asks for
    assert run(stub, nb, env={"HRT_OVERLAP": "1", "HRT_TUNE": "aux_streams=3"}) == log


@pytest.mark.parametrize("mode", ["overlap0", "timer", "nomask", "chain"])
@pytest.mark.parametrize("nb", NB)
def test_no_stream_where_a_trace_must_not_fork_and_the_calls_of_before(stub, golden, mode, nb):
    env, tri, masks, timer = PARENT_MODES[mode]
    for tune in ({}, {"HRT_TUNE": "aux_streams=3"}):
        log = run(stub, nb, tri, masks, timer, 2, dict(env, **tune))
        assert not any(l.startswith("stream_create") or l.startswith("event_create_sync") for l in log), mode
        assert all(l.endswith(" on main") for l in log if " on " in l)
        want = golden["%s/%d" % (mode, nb)]
        # (with a timer the code before made its second stream -- and never used it: the one difference)
        assert log == (_without_aux_objects(want) if mode == "timer" else want)
    if mode == "chain" and nb >= 4:
        assert "chain b0=2 on main" in log


def test_a_stream_of_the_other_priority_is_made_again(stub, tmp_path):
    """HRT_OVERLAP is read by every trace: a stub run cannot change it between two traces, so the two halves are runs
    of their own -- the priority a stream is made at follows the switch of ITS trace"""
    a = [l for l in run(stub, 2) if l.startswith("stream_create")]
    b = [l for l in run(stub, 2, env={"HRT_OVERLAP": "1"}) if l.startswith("stream_create")]
    assert a == ["stream_create lowest -> aux0", "stream_create lowest -> aux1"] and b == ["stream_create default -> aux0"]


def test_the_stub_program_under_the_address_and_undefined_sanitizers(stub, tmp_path):
    """the same program, every case above, with -fsanitize=address,undefined (leaks included): same output, clean exit"""
    san = build_stub(REPO, str(tmp_path / "records_streams_stub_san"), sanitize=True)
    for nb in NB:
        for A in STREAMS:
            env = {"HRT_TUNE": "aux_streams=%d" % A}
            assert run(san, nb, env=env) == run(stub, nb, env=env)
        for m, (env, tri, masks, timer) in PARENT_MODES.items():
            assert run(san, nb, tri, masks, timer, 2, env) == run(stub, nb, tri, masks, timer, 2, env)


if __name__ == "__main__":   # python -m tests.test_records_streams_design <checkout of the commit before>
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = build_stub(sys.argv[1], os.path.join(d, "stub_parent"))
        with open(GOLDEN, "w") as f:
            json.dump(parent_cases(exe), f, indent=0, sort_keys=True)
            f.write("\n")
