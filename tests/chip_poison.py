"""On-chip poison for the GPU tests: run a kernel on LDS and registers it did not write.

A kernel that reads LDS it did not write itself, or a register it did not set, passes every
reference test of this suite when the kernel launched just before it left the right bytes on the
CU -- and in a sweep the sibling variants of one step run back to back on the same data.
``poison()`` launches ``hip_ops.poison_chip()`` on the current stream: every CU's whole 160 KiB
of LDS and every SIMD's 512 vector / accumulator registers hold 0x7FC07FC0 afterwards, a quiet
NaN as bf16, fp16 and fp32. The tests run a call three times on the buffers it writes -- A and
A' plain, P after ``poison()`` -- and require bit-equal results (``same_bits`` / ``bit_diff``: the
tensors are compared as integers, so a NaN equals the same NaN). Imported the way
tests/plan_bound.py and tests/int8_ref.py are; the kernels live in the debug module
(csrc/hip_debug, ``ops/_hip_debug``), which ``build_all()`` builds beside ``_hip``.
``require()`` fails, not skips, where the module is missing, and never compiles inside a test.

The control that the poison bites (tests/test_chip_poison_gpu.py): after ``poison()`` the LDS
probe (every workgroup copies its whole 160 KiB window out without writing it) and the register
probe (a wave holding all 512 registers stores v96, v160, v224, v255, a0, a96, a192 and a255,
none of which it set) must read the pattern in every word of every workgroup, and the probes'
workgroups must have run on every CU and every SIMD of the device (their HW_ID / XCC_ID
registers are recorded). The same probes without a preceding poison are printed only.

Counts and coverage, observed on an MI355X (256 CUs, 1024 SIMDs), poison and probes alike with
256 * 8 = 2048 workgroups of 160 KiB LDS and 256 * 4 * 8 = 8192 waves of 512 registers
(``hip_ops.POISON_LDS_BLOCKS`` / ``POISON_REG_BLOCKS``, the counts ``poison_chip`` always had):
after ``poison()`` 83 886 080 of 83 886 080 probed LDS words (2048 x 40 960) and 4 194 304 of
4 194 304 probed register words (8192 x 8 registers x 64 lanes) held the pattern, and the probes
ran on 256 of 256 CUs and 1024 of 1024 SIMDs: complete, the counts did not have to be raised.
Without a preceding poison 0 of the LDS words held it (informative only).
"""
from __future__ import annotations

import os
import sysconfig

import numpy as np
import torch

PATTERN = 0x7FC07FC0
_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def require():
    """The debug module, or a failure that says how to get it."""
    from semantic_segmentation_server_amd.ops import build
    so = os.path.join(build.HERE, "_hip_debug" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
    assert os.path.exists(so), (f"{so} is missing: the poison tests need the debug extension "
                                "(csrc/hip_debug), which build() / ops.build.build_all() builds")
    from semantic_segmentation_server_amd.ops.native import hip_debug
    mod = hip_debug()
    assert hasattr(mod, "probe_lds") and hasattr(mod, "probe_regs"), f"{so} is stale: it has no probes; run build()"
    return mod


def poison() -> None:
    """Every CU's LDS and every SIMD's VGPR / AGPR file := 0x7FC07FC0, on the current stream."""
    from semantic_segmentation_server_amd.ops import hip_ops
    require()
    hip_ops.poison_chip()


def bit_diff(a: torch.Tensor, b: torch.Tensor):
    """None where ``a`` and ``b`` hold the same bits, else (count of differing elements, first
    differing index)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    ne = a.contiguous().view(_VIEW[a.element_size()]) != b.contiguous().view(_VIEW[b.element_size()])
    if not bool(ne.any()):
        return None
    first = np.unravel_index(int(ne.reshape(-1).int().argmax()), tuple(a.shape))
    return int(ne.sum()), tuple(int(i) for i in first)


def same_bits(got, want, names, what: str):
    """Messages for the tensors of ``got`` that differ in bits from those of ``want``."""
    assert len(got) == len(want) == len(names), (what, len(got), len(want), len(names))
    out = []
    for g, w, n in zip(got, want, names):
        d = bit_diff(torch.as_tensor(g), torch.as_tensor(w))
        if d is not None:
            out.append(f"{n}: {what} at {d[0]} of {torch.as_tensor(g).numel()} elements, first at {d[1]}")
    return out


def _units(ids: torch.Tensor, simd: bool) -> int:
    """Distinct CUs (or SIMDs) among the probes' (HW_ID, XCC_ID) words: SIMD_ID is HW_ID[5:4],
    CU_ID [11:8], SH_ID [12], SE_ID [15:13]; XCC_ID[3:0]."""
    hw, xcc = ids[:, 0].long(), ids[:, 1].long() & 0xF
    key = (xcc << 16) | (hw & 0xFF00) | ((hw & 0x30) if simd else 0)
    return int(key.unique().numel())


def lds_coverage(poisoned: bool):
    """(words that are not the pattern, words probed, distinct CUs the probe ran on, CUs)."""
    from semantic_segmentation_server_amd.ops import hip_ops
    require()
    if poisoned:
        hip_ops.poison_chip()
    words, ids = hip_ops.probe_chip_lds()
    torch.cuda.synchronize()
    bad = int((words != torch.tensor(PATTERN, dtype=torch.int32, device=words.device)).sum())
    return bad, words.numel(), _units(ids, False), torch.cuda.get_device_properties(words.device).multi_processor_count


def reg_coverage(poisoned: bool):
    """(words that are not the pattern, words probed, distinct SIMDs the probe ran on, SIMDs)."""
    from semantic_segmentation_server_amd.ops import hip_ops
    require()
    if poisoned:
        hip_ops.poison_chip()
    words, ids = hip_ops.probe_chip_regs()
    torch.cuda.synchronize()
    bad = int((words != torch.tensor(PATTERN, dtype=torch.int32, device=words.device)).sum())
    return bad, words.numel(), _units(ids, True), 4 * torch.cuda.get_device_properties(words.device).multi_processor_count
