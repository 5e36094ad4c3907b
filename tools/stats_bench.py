"""What the statistics benches share (tools/bench_episode_stats.py, bench_tracking_stats.py, bench_gait_stats.py, bench_push_recovery.py,
bench_step_response.py, bench_frequency_response.py, bench_actuator_stats.py, bench_robustness.py): the timed-call loop and the streaming rate their traffic floors are taken against."""
import statistics

# The rate this project has measured for a streaming kernel of its own: adamw_kernel moves 63.05 MB per launch (profiles/pmc_traffic.json)
# in 15.7 us (profiles/r06zz_rocprofv3_kernel_stats.md) = 4.02 TB/s
STREAM_TBPS = 63.052352 / 15.7     # MB per us = TB/s


def timed_call(call, reps: int, warmup: int, prefix: str = ""):
    """`warmup` untimed calls, then `reps` calls between HIP events: (the median in us, unrounded; {`prefix`us_median, `prefix`us_min,
    `prefix`us_max} rounded to 0.01 us)."""
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    us = statistics.median(ms) * 1e3
    return us, {prefix + "us_median": round(us, 2), prefix + "us_min": round(min(ms) * 1e3, 2), prefix + "us_max": round(max(ms) * 1e3, 2)}


def floor_us(nbytes: float) -> float:
    """The time `nbytes` take at STREAM_TBPS, in us."""
    return nbytes / (STREAM_TBPS * 1e12) * 1e6
