"""The three "merge what is adjacent" loops FusedAdam had before eav_amd.optim._merge_rows replaced them, kept word for
word as the reference of tests/test_optim_plan_cpu.py.  Rows are positional lists of plain integers, as they were:

  merge_ranges   [ptr, other_ptr, numel, slack_bytes]                      accumulate() and clip_grad_norm_
  merge_default  [p, g, m, v, numel, step, gradient tensor, pad_bytes]     step(), once per param group
  merge_jobs     [p, g, m, v, numel, step, lr, wd, pad_bytes]              the multi_tensor step, once over all groups
"""


def merge_ranges(ranges):
    merged = []
    for r in sorted(ranges, key=lambda r: r[0]):
        if merged:
            q = merged[-1]
            gap = r[0] - (q[0] + 4 * q[2])
            if 0 <= gap < q[3] and r[1] - q[1] == r[0] - q[0]:
                q[2] = (r[0] - q[0]) // 4 + r[2]
                q[3] = r[3]
                continue
        merged.append(list(r))
    return merged


def merge_default(runs):
    runs.sort(key=lambda r: r[0])
    merged = []
    for r in runs:
        if merged:
            q = merged[-1]
            gap = r[0] - (q[0] + 4 * q[4])
            if (0 <= gap < 16 + q[7] and r[5] == q[5] and r[1] - q[1] == r[0] - q[0]
                    and r[2] - q[2] == r[0] - q[0] and r[3] - q[3] == r[0] - q[0]):
                q[4] = (r[0] - q[0]) // 4 + r[4]
                q[7] = r[7]
                continue
        merged.append(r)
    return merged


def merge_jobs(runs):
    runs.sort(key=lambda r: r[0])
    jobs = []
    for r in runs:
        if jobs:
            q = jobs[-1]
            gap = r[0] - (q[0] + 4 * q[4])
            if (0 <= gap < 16 + q[8] and r[5:8] == q[5:8] and r[1] - q[1] == r[0] - q[0]
                    and r[2] - q[2] == r[0] - q[0] and r[3] - q[3] == r[0] - q[0]):
                q[4] = (r[0] - q[0]) // 4 + r[4]
                q[8] = r[8]
                continue
        jobs.append(r)
    return jobs
