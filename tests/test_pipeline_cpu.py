"""muavta_amd.pipeline.InFlightRollouts' queue logic over a stub handle (no GPU): a batch with a flagged env fails loudly, leaves the
queue, and the batches behind it — and later submits — carry on.  The same sequence runs on the device in
test_gpu_lanes.py::test_in_flight_pipeline_survives_a_failed_batch."""
import numpy as np
import pytest

from muavta_amd import pipeline
from muavta_amd.native import MuavtaError


class StubEnv:
    """Two state lanes in mode 2, as the pipeline sets them up: each seeded rollout lands on the other lane and only the latest
    batch (back=0) and the one before it (back=1) can be read.  A batch's metrics are its seeds; env flags come from BAD seeds."""
    BAD = {13}

    def __init__(self, config, n_envs, device=0, **kw):
        self.n_envs = n_envs
        self.launched = []
        self.lanes_mode = None
        self.closed = False

    def set_allocator(self, name):
        self.allocator = name

    def set_lanes(self, lanes):
        self.lanes_mode = lanes

    def rollout(self, seeds, n_steps, replan_interval, use_visibility, write_obs):
        assert self.lanes_mode == 2
        self.launched.append(np.asarray(seeds, dtype=np.uint64).copy())

    def _batch(self, back):
        if back not in (0, 1) or back >= len(self.launched):
            raise MuavtaError(f"stub: batch back={back} is gone")
        return self.launched[-1 - back]

    def rollout_metrics(self, back=0):
        return np.repeat(self._batch(back).astype(np.float64)[:, None], 30, axis=1)

    def error_flags(self, back=0):
        return np.array([1 if int(s) in self.BAD else 0 for s in self._batch(back)], dtype=np.int32)

    def close(self):
        self.closed = True


@pytest.fixture
def pipe(monkeypatch):
    monkeypatch.setattr(pipeline, "BatchedMultiUAVEnv", StubEnv)
    p = pipeline.InFlightRollouts(None, 4)
    yield p
    p.close()


def _seeds(first):
    return np.arange(first, first + 4, dtype=np.uint64)


def test_failed_batch_leaves_the_queue_and_carries_its_tag_and_metrics(pipe):
    pipe.submit(_seeds(0), tag="clean0")
    pipe.submit(_seeds(10), tag="bad")  # seed 13 is flagged
    tag, m = next(pipe.results())
    assert tag == "clean0" and np.array_equal(m[:, 0], _seeds(0))
    pipe.submit(_seeds(20), tag="clean1")
    with pytest.raises(MuavtaError) as ei:
        next(pipe.results())
    assert ei.value.tag == "bad"
    assert np.array_equal(ei.value.metrics[:, 0], _seeds(10))
    assert ei.value.error_flags.tolist() == [0, 0, 0, 1]
    pipe.submit(_seeds(30), tag="clean2")  # the failed batch no longer holds a slot
    got = list(pipe.results(all_pending=True))
    assert [t for t, _ in got] == ["clean1", "clean2"]
    assert np.array_equal(got[0][1][:, 0], _seeds(20)) and np.array_equal(got[1][1][:, 0], _seeds(30))
    assert list(pipe.results(all_pending=True)) == []


def test_submit_still_refuses_a_full_queue(pipe):
    pipe.submit(_seeds(0), tag=0)
    pipe.submit(_seeds(4), tag=1)
    with pytest.raises(MuavtaError):
        pipe.submit(_seeds(8), tag=2)
    assert [t for t, _ in pipe.results(all_pending=True)] == [0, 1]


def test_run_stops_at_a_failed_batch_and_the_pipeline_recovers(pipe):
    with pytest.raises(MuavtaError) as ei:
        pipe.run([_seeds(0), _seeds(10), _seeds(20), _seeds(40)])
    assert ei.value.tag == 1
    rest = list(pipe.results(all_pending=True))  # what was queued behind the failed batch is intact
    assert [t for t, _ in rest] == [2]
    assert np.array_equal(rest[0][1][:, 0], _seeds(20))
    assert pipe.run([_seeds(40)])[0][0, 0] == 40
