"""Where the fused finish does not apply, the combine-first finishers give
the buckets they always gave.

TensorAggregator.result_partitions answers None on a CPU (no device table)
and for pass-through frames; SharedPhaseCombiner.finish_buckets and
PartitionWriter.finish then split the aggregator's result frames one by
one, as before the fused finish existed."""

import torch

from bigslice_amd.frame import Frame
from bigslice_amd.kernels.groupby import Options
from bigslice_amd.ops.aggregate import (Aggregation, DictAggregator,
                                        TensorAggregator)
from bigslice_amd.runtime.partition import (PartitionWriter,
                                            SharedPhaseCombiner,
                                            combined_buckets, split_frame)
from bigslice_amd.schema import Schema

SCHEMA = Schema([torch.int64, torch.int64], 1)
NPARTS = 5
CHUNK = 16  # the finishers ask for frames of 4 * CHUNK rows


def _frames(combined_id=None):
    g = torch.Generator().manual_seed(3)
    return [Frame([torch.randint(0, 200, (150,), generator=g),
                   torch.randint(-9, 9, (150,), generator=g)], 1,
                  combined_id=combined_id) for _ in range(3)]


def _old_buckets(agg, chunk):
    buckets = [[] for _ in range(NPARTS)]
    for f in agg.result_frames(chunk * 4):
        for pi, pf in enumerate(split_frame(f, NPARTS, None)):
            if pf is not None and len(pf):
                buckets[pi].append(pf)
    return buckets


def _rows(buckets):
    return [[(f.prefix, [c.tolist() for c in f.columns]) for f in b]
            for b in buckets]


def _fed(frames):
    agg = TensorAggregator(SCHEMA, Aggregation(["sum"]), "cpu")
    for f in frames:
        agg.add(f)
    return agg


def test_options_defaults():
    assert Options.from_env({}) == Options()
    assert Options().sample == "hash" and Options().finish_part
    o = Options.from_env({"BIGSLICE_GB_SAMPLE": "sort",
                          "BIGSLICE_GB_FINISH_PART": "0"})
    assert o.sample == "sort" and not o.finish_part


def test_none_on_cpu():
    assert _fed(_frames()).result_partitions(NPARTS, 64) is None


def test_none_for_pass_through_frames():
    agg = _fed(_frames(combined_id=77))
    assert agg.result_partitions(NPARTS, 64) is None
    assert [f.combined_id for f in agg.result_frames(64)] == [77] * 3


def test_none_leaves_the_aggregator_untouched():
    agg = _fed(_frames())
    assert agg.result_partitions(NPARTS, 64) is None
    assert _rows(_old_buckets(agg, CHUNK)) == \
        _rows(_old_buckets(_fed(_frames()), CHUNK))


def test_aggregator_without_the_method():
    agg = DictAggregator(SCHEMA, Aggregation(["sum"]))
    ref = DictAggregator(SCHEMA, Aggregation(["sum"]))
    for f in _frames():
        agg.add(f)
        ref.add(f)
    assert _rows(combined_buckets(agg, NPARTS, CHUNK * 4)) == \
        _rows(_old_buckets(ref, CHUNK))


def test_partition_writer_buckets_unchanged():
    w = PartitionWriter(NPARTS, None, Aggregation(["sum"]), SCHEMA, "cpu",
                        CHUNK)
    for f in _frames():
        w.add(f)
    got = w.finish()
    want = _old_buckets(_fed(_frames()), CHUNK)
    assert len(got) == NPARTS and sum(len(b) for b in got) > NPARTS
    assert _rows(got) == _rows(want)


def test_shared_phase_combiner_buckets_unchanged():
    for cid in (None, 77):
        sc = SharedPhaseCombiner(SCHEMA, Aggregation(["sum"]), "cpu",
                                 NPARTS, 1, CHUNK)
        for f in _frames(cid):
            sc.add(f)
        assert sc.task_done()
        got = sc.finish_buckets()
        want = _old_buckets(_fed(_frames(cid)), CHUNK)
        assert len(got) == NPARTS
        assert _rows(got) == _rows(want)
