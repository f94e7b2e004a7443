"""Child process of test_gpu_queue_overlap.py: one case per process, because HIP reads GPU_MAX_HW_QUEUES when it initialises.
usage: queue_overlap_child.py two_lanes|one_lane  ->  one JSON line with the measured figures (the parent test asserts on them)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASE, N, STEPS, INTERVAL, QUEUED = "WPS_hard_x2", 256, 150, 20, 8


def queued(h, seeds):
    """QUEUED seeded rollouts without a sync in between, then one sync"""
    for _ in range(QUEUED):
        h.rollout(seeds, STEPS, INTERVAL, True, True)
    h.sync()


def main(mode):
    import torch

    torch.zeros(16, device="cuda").sum().item()  # the framework is up and has used its stream before the handle exists
    from muavta_amd.batched import BatchedMultiUAVEnv
    from muavta_amd.params import params_for_case

    seeds = np.arange(N, dtype=np.uint64)
    two = None
    if mode == "two_lanes":  # the handle under test comes first, right behind the framework: the layout of a process that drives one handle
        two = BatchedMultiUAVEnv(params_for_case(CASE), N)
        two.set_lanes(2)
        queued(two, seeds)
    one = BatchedMultiUAVEnv(params_for_case(CASE), N)
    one.set_lanes(1)
    iso_seed_ms = []
    for _ in range(3):  # isolated launches (the first also allocates the seeding buffers)
        one.rollout(seeds, STEPS, INTERVAL, True, True)
        one.sync()
        iso_seed_ms.append(one.last_seed_ms())
    queued(one, seeds)
    out = {"mode": mode, "queues": os.environ.get("GPU_MAX_HW_QUEUES"), "eager_part_streams": os.environ.get("MUAVTA_EAGER_PART_STREAMS"),
           "one_lane_kernel_ms": one.kernel_ms_history(QUEUED).tolist(), "one_lane_gaps_ms": one.launch_gaps_ms(QUEUED).tolist(),
           "isolated_seed_ms": iso_seed_ms[1:], "one_lane_lanes": list(one.lanes())}
    if mode == "two_lanes":
        want = one.rollout_metrics()
        out["two_lane_lanes"] = list(two.lanes())
        out["two_lane_gaps_ms"] = two.launch_gaps_ms(QUEUED).tolist()
        out["two_lane_kernel_ms"] = two.kernel_ms_history(QUEUED).tolist()
        got = two.rollout_metrics()
        out["metrics_bit_equal"] = bool(got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)))
        out["error_flags"] = int(np.count_nonzero(two.get("ERROR"))) + int(np.count_nonzero(one.get("ERROR")))
        two.close()
    one.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
