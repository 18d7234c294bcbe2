"""CPU checks of the fused image-pooling form: the order table with pool work items, and the
plan structure with and without SSA_POOL_FUSED=0 (plans built on the CPU as in test_plan_cpu)."""
import pytest

from test_plan_cpu import _hip_model, _structure, no_gpu, no_tune, pytestmark as _built  # noqa: F401


def _convs(K, B, BM):
    return [dict(B=B, OH=33, OW=33, k=1, dil=1, Cin=320, Cout=256)] + [
        dict(B=B, OH=33, OW=33, k=3, dil=r, Cin=320, Cout=256, perm=K.tap_group_perm(B, 33, 33, 3, r, BM))
        for r in (6, 12, 18)]


@pytest.mark.parametrize("variant,B,ks,xcds", [(15, 3, 1, 1), (5, 1, 6, 1), (17, 4, 2, 1), (5, 4, 1, 8)])
def test_order_table_with_pool_items(variant, B, ks, xcds):
    """The old table, unchanged and in its order, behind exactly one pool entry per image; the
    (group << 24) | (K slice << 20) | tile fields round-trip, pool entries carry K slice 0."""
    from semantic_segmentation_server_amd.ops import hip_ops as K
    convs = _convs(K, B, K.GROUP_TILE[variant][0])
    old = K.grouped_tile_order(convs, variant, ks=ks, xcds=xcds).tolist()
    new = K.grouped_tile_order(convs, variant, ks=ks, xcds=xcds, pool=B).tolist()
    pool = [e for e in new if e >> 24 == K.POOL_GROUP]
    assert K.POOL_GROUP == 4 and all(e >> 24 < K.POOL_GROUP for e in old)
    assert sorted(e & 0xFFFFF for e in pool) == list(range(B)) and len(new) == len(old) + B
    assert all((e >> 20) & 15 == 0 for e in pool)
    assert sorted(e for e in new if e >> 24 != K.POOL_GROUP) == sorted(old)  # a permutation of the old table
    assert new[B:] == old  # (here: the same order)
    first_gemm = next(i for i, e in enumerate(new) if e >> 24 != K.POOL_GROUP)
    assert first_gemm == B and all(e >> 24 == K.POOL_GROUP for e in new[:B])  # pool items first
    for e in new:
        g, sl, t = e >> 24, (e >> 20) & 15, e & 0xFFFFF
        assert (g << 24) | (sl << 20) | t == e and 0 <= g <= K.POOL_GROUP and sl < ks
    assert K.with_pool_items(K.grouped_tile_order(convs, variant, ks=ks, xcds=xcds), B).tolist() == new


def _branches(ops):
    from semantic_segmentation_server_amd.models.plan import Choice
    return next(op for op in ops if isinstance(op, Choice) and op.name == "aspp.branches")


@_built
def test_plan_offers_fused_forms_after_the_existing_variants(no_tune, monkeypatch):
    """One choice covers branches and pooling: the variants of before, in their order (so pick
    0 and every saved name mean what they meant: separate pooling), each followed by the
    pooling step; then the ``+pool`` forms, one launch each. SSA_POOL_FUSED=0 gives the step
    list of before: the choice without fused forms, then the pooling step."""
    from semantic_segmentation_server_amd.models.plan import Choice
    from semantic_segmentation_server_amd.ops import hip_ops as K
    monkeypatch.delenv("SSA_POOL_FUSED", raising=False)
    ops = _hip_model("mnv2", 2, 129)._plan(2, 120, 160)[0]
    monkeypatch.setenv("SSA_POOL_FUSED", "0")
    ops0 = _hip_model("mnv2", 2, 129)._plan(2, 120, 160)[0]
    br, br0 = _branches(ops), _branches(ops0)
    names, names0 = [n for n, _ in br.variants], [n for n, _ in br0.variants]
    assert names0[-1] == "separate" and not any(n.endswith("+pool") for n in names0)
    assert names[:len(names0)] == names0
    fused = names[len(names0):]
    assert fused == [n + "+pool" for n in names0
                     if n != "separate" and int(n[len("grouped_v"):].split("k")[0]) in K.GROUP_POOL_VARIANTS]
    assert fused and "grouped_v15+pool" in fused and "grouped_v5k6+pool" in fused
    # SSA_POOL_FUSED=0: [.., aspp.branches, pool step, aspp.head, upsample]; fused offered: no
    # top-level pool step, every old variant carries it instead
    i, i0 = ops.index(br), ops0.index(br0)
    assert not isinstance(ops0[i0 + 1], Choice) and isinstance(ops0[i0 + 2], Choice)
    assert ops0[i0 + 2].name == "aspp.head" and ops[i + 1].name == "aspp.head"
    assert len(ops) == len(ops0) - 1
    assert _structure(ops[:i]) == _structure(ops0[:i0]) and _structure(ops[i + 1:]) == _structure(ops0[i0 + 2:])
    for (n, v), (_, v0) in zip(br.variants, br0.variants):
        assert len(v) == len(v0) + 1, n
    assert all(len(v) == 1 for n, v in br.variants if n.endswith("+pool"))


@_built
def test_resnet_plan_keeps_separate_pooling(no_tune, monkeypatch):
    """C = 2048 partials do not fit a pool item's LDS: the ResNet plan has no fused form."""
    monkeypatch.delenv("SSA_POOL_FUSED", raising=False)
    ops = _hip_model("resnet50", 1, 129)._plan(1, 120, 160)[0]
    assert not any(n.endswith("+pool") for n, _ in _branches(ops).variants)
