"""The recorder the launch-trace tools share (encoder_launch_trace.py, eegnet_launch_trace.py): what a step launches, and what it
computes, as one JSON - to compare two commits that should issue the same step (a refactor of the host code): run the tool on
both with the same built library (EAV_LIB_PATH) and diff the files.
A launch is (entry point, scalar arguments) - None kept, an integer >= 2^32 (device addresses, stream handles, 64-bit seeds)
written as "P", every other integer and float as it is; the configurations of one file share most of theirs, so the file holds
every distinct launch once, in `launches` in the order of first use, and each configuration's `step` lists indices into it."""
import hashlib
import json
import os
import sys
from contextlib import contextmanager

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eav_amd import _lib  # noqa: E402


def scalar(a):
    if a is None or isinstance(a, float):
        return a
    a = int(a)
    return "P" if a >= 1 << 32 else a


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@contextmanager
def recording(launches, on=True):
    """Appends every _lib.call inside the block to `launches` (the host code looks `_lib.call` up per launch sequence)."""
    orig = _lib.call

    def call(name, *a):
        launches.append([name, [scalar(v) for v in a]])
        return orig(name, *a)

    if on:
        _lib.call = call
    try:
        yield launches
    finally:
        _lib.call = orig


def encode(result):
    """The JSON text of {configuration: {"launches", "sha256"}}: one distinct launch per line, one configuration per line."""
    dumps = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    index = {}
    steps = {name: [index.setdefault(dumps(launch), len(index)) for launch in r["launches"]] for name, r in result.items()}
    return ('{"launches":[\n' + ",\n".join(index) + '],\n"configurations":{\n'
            + ",\n".join(f'{dumps(name)}:{{"sha256":{dumps(r["sha256"])},"step":{dumps(steps[name])}}}'
                          for name, r in result.items()) + "}}\n")


def write(result, out_path):
    with open(out_path, "w") as f:
        f.write(encode(result))
    print(f"{len(result)} configurations -> {out_path}")
