"""schedule.py's entry for the chained launch (chain14_kernel): the sum of its seven members, and invisible to the unfused totals."""
import pytest

from mermaid_classifier_amd import schedule

CHAIN = "b7.projse-b10.projse.chain"
MEMBERS = ["b7.projse", "b8.mbconv", "b8.projse", "b9.mbconv", "b9.projse", "b10.mbconv", "b10.projse"]


@pytest.mark.parametrize("batch", [1, 128])
def test_chain_entry_is_the_sum_of_its_members(batch):
    ls = schedule.b0_launches(batch)
    by_name = {l.name: l for l in ls}
    assert len(by_name) == len(ls)                       # names are unique: bench.py --full looks launches up by name
    chain = by_name[CHAIN]
    assert chain.kind == "chain"
    assert chain.bytes == sum(by_name[m].bytes for m in MEMBERS) > 0
    assert chain.flops == sum(by_name[m].flops for m in MEMBERS) > 0
    # as launched: the chain in place of its members moves the same bytes and flops
    others = [l.name for l in ls if l.kind in ("stem_dw", "tail")][:1]
    assert schedule.totals(batch, others + [CHAIN]) == schedule.totals(batch, others + MEMBERS)


def test_unfused_totals_do_not_count_the_chain():
    # the values before the chain entry existed
    t1, t128 = schedule.totals(1), schedule.totals(128)
    assert (t1["bytes"], t1["flops"]) == (36914432.0, 769069504.0)
    assert (t128["bytes"], t128["flops"]) == (3514593024.0, 98440896512.0)
    assert t128["bytes_per_patch"] == 27457758.0 and t128["flops_per_patch"] == 769069504.0
    for batch in (1, 128):
        base = [l for l in schedule.b0_launches(batch) if l.kind in ("stem", "expand", "dw", "se", "project", "head")]
        assert schedule.totals(batch)["bytes"] == float(sum(l.bytes for l in base))
        assert schedule.totals(batch)["flops"] == float(sum(l.flops for l in base))
