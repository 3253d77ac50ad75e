"""Writes tests/golden/step_traces.json: the enqueue trace (tests/_trace.py) of one eager step in every configuration of
`tests._trace.configurations()`, on the GPU.  Run it at the commit whose schedule is the reference — a change that is meant to leave the
schedule alone must pass tests/test_gpu_step_trace.py against the file as it is; a change that is meant to move a launch regenerates the
file and shows the move in its diff:

    python tests/golden/make_step_traces.py

Identical traces are stored once: "configs" maps a configuration's name to a trace id, "traces" a trace id to the entries."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import _trace  # noqa: E402


def main():
    cases, ids, configs, traces = {}, {}, {}, {}
    for name, spec in _trace.configurations().items():
        if spec["kind"] not in cases:
            cases[spec["kind"]] = _trace.fit_case(spec["kind"])
        key = json.dumps(_trace.trace_configuration(cases[spec["kind"]]["eng"], spec), separators=(",", ":"))
        if key not in ids:
            ids[key] = "t%03d" % len(ids)
            traces[ids[key]] = key
        configs[name] = ids[key]
    with open(_trace.GOLDEN, "w") as f:                  # one configuration, one trace per line: a regenerated file diffs by line
        f.write('{"configs": {\n' + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in configs.items()) + '\n},\n"traces": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {v}" for k, v in traces.items()) + "\n}}\n")
    print(f"{len(configs)} configurations, {len(traces)} distinct traces, {os.path.getsize(_trace.GOLDEN)} bytes -> {_trace.GOLDEN}")


if __name__ == "__main__":
    main()
