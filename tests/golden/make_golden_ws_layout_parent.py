"""Record every workspace layout and size the engine reports, for tests/test_ws_layout_parent.py (no GPU needed).

Run once with the library whose layouts are the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE a change to the
host code that carves the workspaces):
    python tests/golden/make_golden_ws_layout_parent.py
writes tests/golden/ws_layout_parent.json: "<dtype> B T U1 H V" -> {"layout": {field: value}, "<entry>": [return code, bytes]}.
This module is also the test's source of the cases and of the code that queries them (the test loads it by path).
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, "ws_layout_parent.json")
BTU = [(1, 1, 1), (2, 9, 7), (3, 17, 9), (2, 8, 17), (8, 4000, 601)]
HV = [(64, 32), (64, 28), (128, 128), (384, 256), (640, 512), (640, 768), (1024, 1024)]
DTYPES = ("fp32", "bf16", "bf16x3", "f16x2")
SIZES = ("rnnt_engine_workspace_bytes", "rnnt_engine_loss_workspace_bytes", "rnnt_engine_joint_fwd_workspace_bytes",
         "rnnt_engine_joint_bwd_workspace_bytes")


def cases():
    """(dtype, B, T, U1, H, V): H or V off a multiple of 128 on the fp32 route only."""
    return [(dt, B, T, U1, H, V) for dt in DTYPES for (B, T, U1) in BTU for (H, V) in HV
            if dt == "fp32" or (H % 128 == 0 and V % 128 == 0)]


def key(case):
    return "%s %d %d %d %d %d" % case


def query(engine, case):
    dt, B, T, U1, H, V = case
    lib, code = engine.lib(), engine.dtype_code(dt)
    L = engine.WsLayout()
    assert lib.rnnt_engine_workspace_layout(B, T, U1, H, V, code, ctypes.byref(L)) == 0, key(case)
    out = {"layout": {name: int(getattr(L, name)) for name, _ in engine.WsLayout._fields_}}
    for entry in SIZES:
        n = ctypes.c_size_t(0)
        args = (B, T, U1, V) if entry == "rnnt_engine_loss_workspace_bytes" else (B, T, U1, H, V)
        rc = getattr(lib, entry)(*args, code, ctypes.byref(n))
        out[entry] = [int(rc), int(n.value) if rc == 0 else None]
    return out


def main():
    import rnnt_amd
    rec = {key(c): query(rnnt_amd.engine, c) for c in cases()}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases from %s -> %s (%d bytes)" % (len(rec), rnnt_amd.engine.LIB_PATH, GOLDEN, os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    main()
