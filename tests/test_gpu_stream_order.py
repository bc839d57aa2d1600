"""GPU: every exported function that takes a stream is ordered on that stream (include/monkeypose.h:
"asynchronous on `stream`").  Each case of tests/stream_order_cases.py runs under the hazards H1 - H4
described there -- a late producer, an immediate consumer, an early release of the inputs, two calls back
to back -- on a fresh torch stream and on torch's default stream, and every output must be the bytes of
the plain run (default stream, inputs complete, device sync after).  The plain run itself is held to
float64 or to the host function where the suite does not pin that shape already.

The delay (measured on an MI355X, on the library as it was before this module): host milliseconds for
invoke to return, best of five -- the two-slice pose forward pose-fp32_fft-n64-plain 0.115, bf16 0.113,
frame_pipeline 0.171, detector_pipeline-f32 0.108, regressor-hier-n2 0.391, and the slowest, the dense_hier
graph (regressor-dense_hier-n2, some hundreds of launches, waits and records over its streams), 2.60 =
ENQUEUE_MS.  The rule max(50 ms, 20 x that), capped at 1 s, gives DELAY_MS = 52 ms
(stream_order_cases.DELAY_MS).  The number only has to be comfortably long: the guard is the event recorded
behind the delay, which must still be unfinished after the last enqueue, else the case repeats once at 4 x
the delay and then fails as inconclusive.
"""
import json
import os
import subprocess
import sys

import pytest

import stream_order_cases as SO

ENQUEUE_MS = 2.6        # regressor-dense_hier-n2: host milliseconds for invoke to return, the slowest case


def test_delay_follows_the_rule():
    assert SO.DELAY_MS == min(1000.0, max(50.0, 20.0 * ENQUEUE_MS))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SO.CASES))
def test_call_is_ordered_on_its_stream(name):
    report = SO.run_case(name)
    assert set(report) == {"a fresh stream", "the default stream"}
    for r in report.values():
        assert len(r) == 2 and all("conclusive" in x for x in r), r


@pytest.mark.gpu
@pytest.mark.parametrize("env", SO.CHILD_ENVS, ids=["+".join(f"{k}={v}" for k, v in e.items()) for e in SO.CHILD_ENVS])
def test_pose_slices_in_a_child_process(env):
    """MP_STREAMS=4 MP_SLICE_MIN=16 at n = 64: four slices of 16, so ev_pre is re-recorded three times.
    MP_BB_STAGGER=0: the side slice's backbone waits for ev_fork alone.  The switches are read once per
    process: one child at a time, which runs the same harness."""
    r = subprocess.run([sys.executable, os.path.join(SO.ROOT, "tests", "stream_order_cases.py"), SO.CHILD_CASE],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    report = json.loads(r.stdout.strip().splitlines()[-1])["report"]
    print(env, report)
    assert set(report) == {"a fresh stream", "the default stream"}
    for x in report.values():
        assert len(x) == 2 and all("conclusive" in y for y in x), x


@pytest.mark.gpu
def test_two_contexts_on_two_streams():
    """a pose context on one stream and a dense graph context on another, each behind its own delayed
    producer, enqueued interleaved: the two share no device state, so each equals its plain run"""
    assert len(SO.run_two_contexts()) == 2
