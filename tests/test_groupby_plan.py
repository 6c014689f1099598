"""The group-by combiner's decisions, as plain arithmetic on a CPU.

The chooser, the partitioned-insert plan and the regrow rule carry a
tuning that was won by measurement on the GPU.  Every expected value
below was produced by the implementation that preceded these functions
(GroupTable._read_sample and the inline rules of _insert_now and finish
at commit 09644e3), so a change to the tuning has to change this file.
"""

import pytest
import torch

from bigslice_amd.kernels.groupby import (GroupTable, Options, choose_mode,
                                          forced_mode, part_plan,
                                          regrow_capacity)

S = 1 << 19            # sample rows
BATCH = 7_812_500      # rows of one flagship batch (125M / 16)
AUTO = Options()

# geometry of csrc/groupby_part.hip: LDS slots, tile rows, max buckets
GEOM = (4096, 8192, 1024)
MIN_ROWS = 1 << 21


def choose(distinct, batch=BATCH, sum_i64=True, opts=AUTO, cap_hint=None):
    return choose_mode(distinct, S, batch, sum_i64, opts, cap_hint)


# sampled distinct keys of 2^19 rows -> (mode, cap_hint, key estimate)
@pytest.mark.parametrize("distinct,mode,cap_hint,estimate", [
    (1000, "lds", 4096, 1000.0),
    (16384, "lds", 65536, 16384.000000000207),
    (16385, "part", 131072, 16385.000000000207),
    (65514, "part", 262144, 65535.98483299057),         # 64k keys
    (408023, "part", 4194304, 997716.5513713078),       # 1M keys
    (412711, "part", 4194304, 1046779.7851145716),      # 1.05M keys
    (413604, "part", 8388608, 1056563.8450130932),      # 1.06M: the cliff
    (461373, "global", 8388608, 1905978.1683394173),
    (461374, "sort", 8388608, 1906005.9728575149),
    # 10M keys: the fixed point has not converged after 20 steps
    (510781, "sort", 33554432, 4505383.778034276),
    (524287, "sort", 33554432, 5986876.5833150735),
    (524288, "sort", None, None),                       # saturated
])
def test_chooser_bands(distinct, mode, cap_hint, estimate):
    got_mode, got_estimate, got_hint = choose(distinct)
    assert got_mode == mode
    assert got_hint == cap_hint
    if estimate is None:
        assert got_estimate is None
    else:
        assert got_estimate == pytest.approx(estimate, rel=1e-9)


def test_chooser_rows_per_key_band():
    # 64k keys, 40M-row batch: more than 500 rows per key
    assert choose(65514, batch=40_000_000)[::2] == ("sort", 262144)
    # 1M keys, 5M-row batch: under 6 rows per key
    assert choose(408023, batch=5_000_000)[::2] == ("global", 4194304)
    # the band's lower edge at 1M keys sits between these two batches
    assert choose(408023, batch=5_986_302)[0] == "part"
    # "part" is for the single int64 sum only
    assert choose(408023, sum_i64=False)[::2] == ("global", 4194304)


def test_chooser_part_disabled():
    opts = Options.from_env({"BIGSLICE_GB_PART": "0"})
    assert choose(408023, opts=opts)[::2] == ("global", 4194304)
    assert choose(1000, opts=opts)[0] == "lds"


def test_chooser_keeps_caller_cap_hint():
    mode, estimate, hint = choose(408023, cap_hint=2048)
    assert (mode, hint) == ("part", 2048)
    assert estimate == pytest.approx(997716.5513713078, rel=1e-9)


@pytest.mark.parametrize("env,sum_i64,want", [
    ({"BIGSLICE_GB_MODE": "lds"}, True, "lds"),
    ({"BIGSLICE_GB_MODE": "lds"}, False, "lds"),
    ({"BIGSLICE_GB_MODE": "global"}, True, "global"),
    ({"BIGSLICE_GB_MODE": "part"}, False, "global"),
    ({"BIGSLICE_GB_COMBINE": "sort"}, True, "sort"),
    # the mode wins over the combine
    ({"BIGSLICE_GB_MODE": "lds", "BIGSLICE_GB_COMBINE": "sort"}, True, "lds"),
    ({"BIGSLICE_GB_MODE": "part", "BIGSLICE_GB_COMBINE": "sort"}, True,
     "sort"),
    ({"BIGSLICE_GB_MODE": "global", "BIGSLICE_GB_COMBINE": "hash"}, True,
     "global"),
])
def test_forced_without_sample(env, sum_i64, want):
    opts = Options.from_env(env)
    assert forced_mode(opts, sum_i64) == want
    # whatever the sample says, and without an estimate or a hint
    for distinct in (1000, 408023, 524288):
        assert choose(distinct, sum_i64=sum_i64, opts=opts) == (
            want, None, None)


@pytest.mark.parametrize("env", [
    {}, {"BIGSLICE_GB_MODE": "auto"}, {"BIGSLICE_GB_MODE": "part"},
    {"BIGSLICE_GB_COMBINE": "hash"}, {"BIGSLICE_GB_COMBINE": "auto"}])
def test_sampling_settings_force_nothing(env):
    assert forced_mode(Options.from_env(env), True) is None


def test_forced_part_still_sizes_from_the_sample():
    opts = Options.from_env({"BIGSLICE_GB_MODE": "part"})
    assert choose(1000, opts=opts) == ("part", 1000.0, 4096)
    mode, estimate, hint = choose(510781, opts=opts)
    assert (mode, hint) == ("part", 33554432)
    assert estimate == pytest.approx(4505383.778034276, rel=1e-9)
    assert choose(524288, opts=opts) == ("part", None, None)


def test_combine_hash_turns_sort_into_global():
    opts = Options.from_env({"BIGSLICE_GB_COMBINE": "hash"})
    # saturated sample, the 88% threshold, and >500 rows per key
    assert choose(524288, opts=opts) == ("global", None, None)
    assert choose(461374, opts=opts)[::2] == ("global", 8388608)
    assert choose(65514, batch=40_000_000, opts=opts)[::2] == (
        "global", 262144)
    # every other verdict is the ordinary chooser's
    for distinct in (1000, 16385, 408023, 461373):
        assert choose(distinct, opts=opts) == choose(distinct)


def test_options_from_env():
    assert Options.from_env({}) == AUTO
    opts = Options.from_env({
        "BIGSLICE_GB_MODE": "part", "BIGSLICE_GB_COMBINE": "hash",
        "BIGSLICE_GB_PART": "0", "BIGSLICE_GB_PART_OWNED": "0",
        "BIGSLICE_GB_LDS_BLOCKS": "512", "BIGSLICE_GB_SAMPLE_ROWS": "4096",
        "BIGSLICE_GB_DEBUG": "1"})
    assert opts == Options(mode="part", combine="hash", part=False,
                           part_owned=False, lds_blocks=512,
                           sample_rows=4096, debug=True)


def test_table_reads_environment_once(monkeypatch):
    monkeypatch.setenv("BIGSLICE_GB_MODE", "global")
    t = GroupTable([torch.int64], ["sum"], "cpu")
    monkeypatch.setenv("BIGSLICE_GB_MODE", "lds")
    assert t.opts.mode == "global"
    assert GroupTable([torch.int64], ["sum"], "cpu").opts.mode == "lds"


def test_table_applies_the_choice(monkeypatch):
    for name in ("BIGSLICE_GB_MODE", "BIGSLICE_GB_COMBINE",
                 "BIGSLICE_GB_PART"):
        monkeypatch.delenv(name, raising=False)
    t = GroupTable([torch.int64], ["sum"], "cpu")
    assert t._mode is None and t._key_estimate is None
    t._sample_n, t._sample_batch_n = S, BATCH
    t._sample_ne = torch.tensor(408023 - 1)
    assert t._read_sample() == "part"
    assert t.cap_hint == 4194304
    assert t._key_estimate == pytest.approx(997716.5513713078, rel=1e-9)
    # a caller's hint stays
    t = GroupTable([torch.float32], ["sum"], "cpu", cap_hint=2048)
    t._sample_n, t._sample_batch_n = S, BATCH
    t._sample_ne = torch.tensor(408023 - 1)
    assert t._read_sample() == "global"
    assert t.cap_hint == 2048


def plan(n, cap, estimate, opts=AUTO, min_rows=MIN_ROWS):
    return part_plan(n, cap, estimate, opts, *GEOM, min_rows)


def test_part_plan():
    owned_off = Options.from_env({"BIGSLICE_GB_PART_OWNED": "0"})
    # flagship batch into the 1M-key table: owned slices of 4096 slots
    assert plan(BATCH, 1 << 22, 997716.55) == ("owned", 1024)
    # past the cliff a slice would need 8192 slots: the tiled pass
    assert plan(BATCH, 1 << 23, 1056563.8) == ("tiled", 1024)
    # 64k keys: the owned pass at the row count's fan-out, or the
    # tiled pass at the key count's
    assert plan(8 << 20, 1 << 18, 65536.0) == ("owned", 1024)
    assert plan(8 << 20, 1 << 18, 65536.0, owned_off) == ("tiled", 64)
    # no estimate (forced mode, saturated sample): a quarter of the table
    assert plan(8 << 20, 1 << 18, None, owned_off) == ("tiled", 64)
    # small and oversize batches take the plain insert
    assert plan(MIN_ROWS - 1, 1 << 22, 997716.55) is None
    assert plan(MIN_ROWS, 1 << 22, 997716.55) == ("owned", 1024)
    assert plan((1 << 31) - 1, 1 << 22, 997716.55) == ("owned", 1024)
    assert plan(1 << 31, 1 << 22, 997716.55) is None
    assert plan(1000, 1024, None, min_rows=1) == ("owned", 2)


def test_regrow_capacity():
    # four slots per row so far
    assert regrow_capacity(1024, 3_000_000) == 1 << 24
    assert regrow_capacity(1 << 22, (1 << 20) + 1) == 1 << 23
    # already that large: double anyway (the overflow was real)
    assert regrow_capacity(1 << 24, 1000) == 1 << 25
    assert regrow_capacity(1 << 22, 1 << 20) == 1 << 23
    # the row target stops at 2^30; one more doubling is allowed
    assert regrow_capacity(1 << 20, 1 << 40) == 1 << 30
    assert regrow_capacity(1 << 30, 1 << 40) == 1 << 31
    with pytest.raises(RuntimeError, match="groupby table overflow"):
        regrow_capacity(1 << 31, 1 << 40)
