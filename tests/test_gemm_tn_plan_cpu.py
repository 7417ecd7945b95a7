"""CPU-only checks of the weight-gradient product's planning entries (mtmp_gemm_tn_slab_rows, mtmp_gemm_tn_ws_floats) for
the widths of the trainable image encoder, which are not multiples of 128, and for three 128-multiple shapes whose plan must
not move.  The entries are pure host code; the library loads without a GPU.  Every ctypes call runs in a child process: a
planner that divides by a tile count of zero ends that child with SIGFPE, which fails one test instead of the session."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "medical_tri_modal_pilot_amd", "libmtmp_hip.so")

# (N = dY width, K = X width) of the ten weight gradients of the stem, stages 1-2 and patch merging 1
ENCODER_SHAPES = [(96, 16), (288, 96), (96, 96), (384, 96), (96, 384), (192, 384), (576, 192), (192, 192), (768, 192), (192, 768)]
ENCODER_M = [7, 3136, 200704]
# 128-multiple shapes at M = 64320 and the plan of the commit before the encoder widths were added:
# (N, K) -> (ws_floats, slab_rows dtype 0, slab_rows dtype 1)
TUNED_M = 64320
TUNED_PLAN = {(768, 256): (10460928, 53, 16), (256, 1024): (10496000, 40, 12), (1024, 256): (10526720, 40, 12)}

_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.mtmp_gemm_tn_ws_floats.restype = ctypes.c_longlong
lib.mtmp_gemm_tn_ws_floats.argtypes = [ctypes.c_int] * 3
lib.mtmp_gemm_tn_slab_rows.restype = ctypes.c_int
lib.mtmp_gemm_tn_slab_rows.argtypes = [ctypes.c_int] * 4
out = []
for M, N, K in json.loads(sys.argv[2]):
    out.append([M, N, K, lib.mtmp_gemm_tn_ws_floats(M, N, K), lib.mtmp_gemm_tn_slab_rows(0, M, N, K),
                lib.mtmp_gemm_tn_slab_rows(1, M, N, K)])
print(json.dumps(out))
"""


def _plan(cases):
    """[(M, N, K)] -> {(M, N, K): (ws_floats, slab_rows fp32, slab_rows bf16)}, computed in a child process"""
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    r = subprocess.run([sys.executable, "-c", _CHILD, LIB, json.dumps(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, f"planning child ended with status {r.returncode} (-8: SIGFPE)\n{r.stderr[-2000:]}"
    return {tuple(e[:3]): tuple(e[3:]) for e in json.loads(r.stdout.strip().splitlines()[-1])}


@pytest.mark.parametrize("N,K", ENCODER_SHAPES)
def test_plan_covers_encoder_widths(N, K):
    plan = _plan([(M, N, K) for M in ENCODER_M])
    for M in ENCODER_M:
        ws, rows0, rows1 = plan[(M, N, K)]
        print(f"M={M} N={N} K={K}: ws_floats {ws} slab_rows fp32 {rows0} bf16 {rows1}")
        for rows in (rows0, rows1):
            assert rows >= 1
            assert ws >= rows * (N * K + N)


def test_plan_of_128_multiples_is_unchanged():
    plan = _plan([(TUNED_M, N, K) for N, K in TUNED_PLAN])
    for (N, K), want in TUNED_PLAN.items():
        got = plan[(TUNED_M, N, K)]
        print(f"M={TUNED_M} N={N} K={K}: {got} (before: {want})")
        assert got == want
        assert got[0] >= max(got[1:]) * (N * K + N)
