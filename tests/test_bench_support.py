"""CPU tests of tools/bench_support.py, what the thirteen tools/batch_*_bench.py share: every tool imports without a GPU; the
input functions give, bit for bit, the arrays their copies gave before they were merged (SHA-256 of the array bytes, recorded from
the copies in the tools of the commit before the merge: there the four copies of the fleet and the two of the inputs agreed);
stats and summary on hand-made rounds; and the two loops, driven by a handle that records its calls, make the call sequences
that the tools' own loops made -- the expected lists are written out from tools/batch_shift_bench.py (measure, resident_tick) and
tools/batch_scan_bench.py (resident_tick, the costmap form) of that commit.  Nothing of the GPU side is touched."""
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import bench_support as bs  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402

TOOLS = ("batch_bench", "batch_resident_bench", "batch_params_bench", "batch_shift_bench", "batch_obstacles_bench",
         "batch_moving_bench", "batch_grid_bench", "batch_fleet_bench", "batch_feed_bench", "batch_costmap_bench", "batch_roll_bench",
         "batch_scan_bench", "batch_sense_bench")


def test_every_tool_imports_without_a_gpu(monkeypatch):
    def touched(*_a, **_k):
        raise AssertionError("a bench tool reached torch.cuda while it was imported")

    had_torch = "torch" in sys.modules
    if had_torch:
        cuda = sys.modules["torch"].cuda
        for name in ("_lazy_init", "init", "get_device_properties", "Stream", "Event", "synchronize"):
            monkeypatch.setattr(cuda, name, touched)
    for name in TOOLS:
        sys.modules.pop(name, None)
        tool = importlib.import_module(name)
        assert callable(tool.main) and tool.bs is bs, name
    assert had_torch or "torch" not in sys.modules


# ---- the inputs, pinned --------------------------------------------------------------------------------------------------------------
def _digest(x):
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, (list, tuple)):
            for w in v:
                feed(w)
        else:
            h.update(np.ascontiguousarray(v).tobytes())

    feed(x)
    return h.hexdigest()


B = 5
PINNED = {   # model: (configuration, fleet(p, B), inputs(p, B))
    "diff_drive": (configs.diff_drive_defaults(1000, 15), "cdd14417f044eadae13d60c9f8f8915f94a85d05d88c69edf8e09612025ef5e0",
                   "c11d0bab1f088b294ba413cfa8db5f2096b00a7f4db9bb9f3c7b265cf262ca8a"),
    "steering": (configs.steering_defaults(10000, 15), "cdd14417f044eadae13d60c9f8f8915f94a85d05d88c69edf8e09612025ef5e0",
                 "c11d0bab1f088b294ba413cfa8db5f2096b00a7f4db9bb9f3c7b265cf262ca8a"),
    "full_body": (configs.full_body_defaults(10000, 15), "a2ba4e4cad69124bf0683e01f2c5669d6dcd26e98921a406ccc375cae8a71e0d",
                  "ab095c215c382f1271e34783d36b0c6b8e5e9526e49366d76761fc9c293a40ee"),
}


@pytest.mark.parametrize("model", sorted(PINNED))
def test_fleet_and_inputs_are_the_arrays_of_the_copies_they_replace(model):
    p, fleet, inputs = PINNED[model]
    assert _digest(bs.fleet(p, B)) == fleet
    assert _digest(bs.inputs(p, B)) == inputs


def test_scatter_velocities_and_layer_at_their_default_seeds():
    s0 = bs.fleet(PINNED["diff_drive"][0], B)[1]
    assert _digest(bs.scatter(s0[:, :2], 8)) == "c2782b560ac4e4df75d30852803c22fb305b33eb6a98f69cf4292146cc592265"
    assert _digest(bs.velocities(B, 8)) == "8df22eb791cd75fed13625447dc8a4dd4e4c6153f11e5121a5acec4bb0630729"
    assert _digest(bs.layer(40, 30)) == "d6d075b413a42784850937491ba4a4b2bfd0292879692b446bb952f03a3c06bf"
    assert bs.layer(40, 30).shape == (30, 40) and len(bs.scatter(s0[:, :2], 8)) == B and bs.velocities(B, 8)[0].shape == (8, 2)


def test_tracking_errors_on_a_hand_made_trace():
    px, py = np.array([0.0, 1.0, 2.0]), np.zeros(3)
    trace = np.array([[0.0, 0.0, 0.0], [1.0, 3.0, 0.0], [2.0, -4.0, 0.0]])
    assert bs.tracking_errors(trace, px, py) == (4.0, float(np.sqrt(25.0 / 3.0)))
    assert bs.travelled(trace) == float(np.hypot(2.0, 4.0))


# ---- summaries -----------------------------------------------------------------------------------------------------------------------
def test_stats_median_rounds_and_the_spread_of_a_baseline_only():
    assert bs.stats([3.0, 1.0, 8.0]) == {"median": 3.0, "rounds": [3.0, 1.0, 8.0]}
    assert bs.stats([3.0, 1.0, 8.0], True) == {"median": 3.0, "rounds": [3.0, 1.0, 8.0], "spread": 7.0}
    out = {}
    bs.tick_stats(out, {"none": [1.0, 2.0], "scan": [5.0, 3.0]}, {"none": [2.0, 4.0], "scan": [6.0, 6.0]})
    assert out == {"none_tick_us": {"median": 1.5, "rounds": [1.0, 2.0], "spread": 1.0}, "scan_tick_us": {"median": 4.0, "rounds": [5.0, 3.0]},
                   "none_wall_us": {"median": 3.0, "rounds": [2.0, 4.0], "spread": 2.0}, "scan_wall_us": {"median": 6.0, "rounds": [6.0, 6.0]}}


def test_summary_medians_and_spreads_of_the_baseline_mode_with_the_unit_suffix():
    times = {"off_kernel": [4.0, 1.0, 2.0], "on_kernel": [9.0, 5.0, 7.0], "off_iter": [10.0, 30.0, 20.0], "on_iter": [11.0, 12.0, 13.0]}
    res = {"B": 1}
    bs.summary(res, times, "_us")
    assert res == {"B": 1, "per_round": {"off_kernel_us": [4.0, 1.0, 2.0], "on_kernel_us": [9.0, 5.0, 7.0], "off_iter_us": [10.0, 30.0, 20.0],
                                         "on_iter_us": [11.0, 12.0, 13.0]},
                   "off_kernel_us": 2.0, "on_kernel_us": 7.0, "off_iter_us": 20.0, "on_iter_us": 12.0,
                   "spread_off_kernel_us": 3.0, "spread_off_iter_us": 20.0}
    res = {}
    bs.summary(res, {"static_n8": [1.0, 2.0], "moving_n8": [3.0, 5.0]}, "_tick_us", baseline="static")
    assert res == {"per_round": {"static_n8_tick_us": [1.0, 2.0], "moving_n8_tick_us": [3.0, 5.0]}, "static_n8_tick_us": 1.5,
                   "moving_n8_tick_us": 4.0, "spread_static_n8_tick_us": 1.0}
    res = {}
    bs.summary(res, {"shared": [1.0, 3.0]}, "_kernel_us", baseline=None)
    assert res == {"per_round": {"shared_kernel_us": [1.0, 3.0]}, "shared_kernel_us": 2.0}


def test_parser_defaults_and_the_written_document(tmp_path, capsys):
    a = bs.parser("batch_sense_bench.json", ticks=40, warmup=10).parse_args([])
    assert (a.rounds, a.warmup, a.ticks) == (3, 10, 40) and not hasattr(a, "iters")
    assert a.out == os.path.join(bs.ROOT, "profiles", "batch_sense_bench.json")
    a = bs.parser(None, iters=256).parse_args(["--rounds", "2"])
    assert (a.iters, a.rounds, a.warmup, a.out) == (256, 2, 20, None) and not hasattr(a, "ticks")
    a = bs.parser("x.json", iters=256, ticks=256, rounds=5).parse_args([])
    assert (a.iters, a.rounds, a.warmup, a.ticks) == (256, 5, 20, 256)
    path = tmp_path / "sub" / "doc.json"
    bs.emit({"a": [1, 2]}, str(path))
    assert path.read_text() == capsys.readouterr().out == '{\n "a": [\n  1,\n  2\n ]\n}\n'


# ---- the loops, by a handle that records its calls ---------------------------------------------------------------------------------
class Recorder:
    """every method call goes to `log` as (name, args) or, with keywords, (name, args, kwargs)"""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*args, **kwargs):
            self.log.append((name, args, kwargs) if kwargs else (name, args))
            return {"timing_read": (30.0, 60.0, 3), "last_kernel": 7}.get(name)
        return call


@pytest.fixture
def log(monkeypatch):
    """the call log; the module's one way to torch is a counter that writes its events to the same log"""
    log, clock = [], [0]

    def event_pair(stream=None, idle_device=False):
        log.append(("events", (stream, idle_device)))

        def elapsed_us():
            clock[0] += 1
            return 600.0 * clock[0]

        return (lambda: log.append(("start", ()))), (lambda: log.append(("stop", ()))), elapsed_us

    monkeypatch.setattr(bs, "event_pair", event_pair)
    return log


NOSTATS = {"want_stats": False}


def test_measure_modes_makes_the_calls_of_the_shift_tools_measure(log):
    h = Recorder(log)
    modes = (("off", False), ("on", True))
    times, kernel = bs.measure_modes(h, ("INS",), modes, lambda h, mode: h.set_min_shift(mode[1]), iters=3, rounds=2, warmup=2)
    assert log == [
        ("set_min_shift", (False,)), ("iterate", ("INS", 0), NOSTATS), ("iterate", ("INS", 1), NOSTATS),
        ("set_min_shift", (True,)), ("iterate", ("INS", 0), NOSTATS), ("iterate", ("INS", 1), NOSTATS),
        # round 0
        ("set_min_shift", (False,)), ("timing_enable", (True,)), ("iterate_enqueue", ("INS", 0)), ("iterate_enqueue", ("INS", 1)),
        ("iterate_enqueue", ("INS", 2)), ("timing_read", ()), ("timing_enable", (False,)), ("last_kernel", ()),
        ("set_min_shift", (True,)), ("timing_enable", (True,)), ("iterate_enqueue", ("INS", 0)), ("iterate_enqueue", ("INS", 1)),
        ("iterate_enqueue", ("INS", 2)), ("timing_read", ()), ("timing_enable", (False,)), ("last_kernel", ()),
        # round 1
        ("set_min_shift", (False,)), ("timing_enable", (True,)), ("iterate_enqueue", ("INS", 3)), ("iterate_enqueue", ("INS", 4)),
        ("iterate_enqueue", ("INS", 5)), ("timing_read", ()), ("timing_enable", (False,)), ("last_kernel", ()),
        ("set_min_shift", (True,)), ("timing_enable", (True,)), ("iterate_enqueue", ("INS", 3)), ("iterate_enqueue", ("INS", 4)),
        ("iterate_enqueue", ("INS", 5)), ("timing_read", ()), ("timing_enable", (False,)), ("last_kernel", ()),
    ]
    assert times == {"off_kernel": [10.0, 10.0], "off_iter": [20.0, 20.0], "on_kernel": [10.0, 10.0], "on_iter": [20.0, 20.0]}
    assert kernel == {"off": 7, "on": 7}


def test_measure_modes_hands_every_kernel_to_the_check(log):
    seen = []
    bs.measure_modes(Recorder(log), (), ("off", "small"), lambda h, mode: None, iters=1, rounds=2, warmup=0,
                     check=lambda mode, kernel: seen.append((mode, kernel)))
    assert seen == [("off", 7), ("small", 7), ("off", 7), ("small", 7)]


ADVANCE, HOLD = {"advance": True}, {"advance": False}


def test_resident_modes_makes_the_calls_of_the_shift_tools_resident_tick(log):
    h = Recorder(log)
    modes = (("off", False), ("on", True))
    times, _wall, kernel = bs.resident_modes(h, "STREAM", "S0", "SEEDS", 0.1, modes, lambda h, mode: h.set_min_shift(mode[1]),
                                             ticks=3, rounds=2, warmup=2)
    one = lambda on: [
        ("set_min_shift", (on,)), ("resident_set_poses", ("S0", "SEEDS")),
        ("resident_step_enqueue", (0.1, 0), HOLD), ("resident_step_enqueue", (0.1, 1), ADVANCE),
        ("events", ("STREAM", False)), ("start", ()),
        ("resident_step_enqueue", (0.1, 2)), ("resident_step_enqueue", (0.1, 3)), ("resident_step_enqueue", (0.1, 4)),
        ("stop", ()), ("last_kernel", ())]
    assert log == one(False) + one(True) + one(False) + one(True)
    assert times == {"off": [200.0, 600.0], "on": [400.0, 800.0]} and kernel == {"off": 7, "on": 7}


def test_resident_modes_costmap_form_makes_the_calls_of_the_scan_tools_resident_tick(log):
    h = Recorder(log)
    seen = []
    times, wall, _kernel = bs.resident_modes(h, "STREAM", "S0", "SEEDS", 0.1, ("none", "scan"), lambda h, mode: h.set_occupancy("OCC"),
                                             ticks=3, rounds=2, warmup=2, after_step=lambda mode, i: mode == "scan" and h.scan(i % 16),
                                             costmap_form=True, check=lambda mode, kernel: seen.append((mode, kernel)))
    head = [("set_occupancy", ("OCC",)), ("resident_set_poses", ("S0", "SEEDS")),
            ("resident_step_enqueue", (0.1, 0), HOLD), ("resident_step_enqueue", (0.1, 1), ADVANCE),
            ("synchronize", ()), ("events", ("STREAM", False)), ("start", ())]
    none = head + [("resident_step_enqueue", (0.1, 2)), ("resident_step_enqueue", (0.1, 3)), ("resident_step_enqueue", (0.1, 4)),
                   ("stop", ()), ("last_kernel", ())]
    scan = head + [("resident_step_enqueue", (0.1, 2)), ("scan", (0,)), ("resident_step_enqueue", (0.1, 3)), ("scan", (1,)),
                   ("resident_step_enqueue", (0.1, 4)), ("scan", (2,)), ("stop", ()), ("last_kernel", ())]
    assert log == none + scan + none + scan
    assert times == {"none": [200.0, 600.0], "scan": [400.0, 800.0]} and seen == [("none", 7), ("scan", 7)] * 2
    assert set(wall) == {"none", "scan"} and all(len(v) == 2 and min(v) >= 0.0 for v in wall.values())


def test_resident_modes_enqueues_a_modes_work_before_the_step_too(log):
    """the costmap and roll tools' baseline: the parent's whole-map call before every step, inside the timed region"""
    h = Recorder(log)
    bs.resident_modes(h, "STREAM", "S0", "SEEDS", 0.1, ("set_grids",), lambda h, mode: None, ticks=2, rounds=1, warmup=0,
                      before_step=lambda mode, i: h.set_grids(i), costmap_form=True)
    assert log == [("resident_set_poses", ("S0", "SEEDS")), ("synchronize", ()), ("events", ("STREAM", False)), ("start", ()),
                   ("set_grids", (0,)), ("resident_step_enqueue", (0.1, 0)), ("set_grids", (1,)), ("resident_step_enqueue", (0.1, 1)),
                   ("stop", ()), ("last_kernel", ())]


def test_tick_us_brackets_the_ticks_and_one_call_times_it_twice(log):
    h = Recorder(log)
    assert bs.tick_us("STREAM", 4, lambda i: h.tick(i)) == 150.0
    assert log == [("events", ("STREAM", False)), ("start", ()), ("tick", (0,)), ("tick", (1,)), ("tick", (2,)), ("tick", (3,)), ("stop", ())]
    del log[:]
    ms, us = bs.one_call_ms_and_us(h, "STREAM", 2, lambda: h.there(), lambda: h.back())
    assert log == 2 * [("there", ()), ("synchronize", ()), ("events", ("STREAM", False)), ("start", ()), ("back", ()), ("stop", ())]
    assert us == {"median": 1500.0, "rounds": [1200.0, 1800.0]} and len(ms["rounds"]) == 2


def test_idle_call_us_synchronises_before_fewer_calls_than_slots(log):
    h = Recorder(log)
    got = bs.idle_call_us(h, lambda i: h.patch(i), rounds=1)
    burst = [("synchronize", ())] + [("patch", (i,)) for i in range(capi.OCC_PATCH_SLOTS - 1)]
    assert log == 8 * burst and len(got["rounds"]) == 7 and "spread" not in got


def test_closed_loop_drives_reads_every_trace_and_reports(log):
    h = Recorder(log)
    px, py = np.array([0.0, 1.0, 2.0]), np.zeros(3)
    traces = [np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.0]]), np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])]
    h.resident_read_trace = lambda b: (log.append(("resident_read_trace", (b,))), traces[b])[1]
    s0 = np.zeros((2, 3))
    legs, us = bs.closed_loop(h, (px, py), s0, "SEEDS", 0.1, 3, lambda b, tr, finite: {"robot": b}, timed=True)
    assert log == [("resident_set_paths", ((px, py),)), ("resident_set_poses", (s0, "SEEDS")), ("events", (None, True)), ("start", ()),
                   ("resident_step_enqueue", (0.1, 0), HOLD), ("resident_step_enqueue", (0.1, 1), ADVANCE),
                   ("resident_step_enqueue", (0.1, 2), ADVANCE), ("synchronize", ()), ("stop", ()),
                   ("resident_read_trace", (0,)), ("resident_read_trace", (1,))]
    assert us == 200.0 and legs[0] == {"finite": True, "max_m": 1.0, "rms_m": float(np.sqrt(0.5)), "robot": 0}
    assert legs[1]["finite"] is False and np.isnan(legs[1]["max_m"]) and np.isnan(legs[1]["rms_m"]) and legs[1]["robot"] == 1
    del log[:]
    assert len(bs.closed_loop(h, (px, py), s0, "SEEDS", 0.1, 1, lambda b, tr, finite: {})) == 2 and ("start", ()) not in log
