"""mog_air.summaries on the host: the bucket limits, the histogram encoding,
the event file (read back by the project's own record reader and, a second
time, by google.protobuf with descriptors built here from the field numbers
the module states), the numeric tags against the reference's naming rule, and
the argument refusals."""
import argparse
import glob
import math
import struct
import sys

import numpy as np
import pytest

import summary_ref as ref
from mog_air import records, summaries


# ---------------------------------------------------------------- limits ----
def test_bucket_limits():
    lim = summaries.bucket_limits()
    assert lim.shape == (1551,) and lim.dtype == np.float64
    assert np.all(np.diff(lim) > 0)
    assert lim[0] == -sys.float_info.max and lim[-1] == sys.float_info.max
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[774] == -1e-12
    assert np.array_equal(lim, ref.limits())


def test_no_limit_is_a_float32_and_thresholds_classify_exactly():
    pos = ref.positive_limits()
    assert len(pos) == 774
    assert not np.any(pos.astype(np.float32).astype(np.float64) == pos)
    thr = summaries.bucket_thresholds()
    assert thr.dtype == np.float32 and thr.shape == (774,) and np.all(np.diff(thr) > 0)
    below = np.nextafter(thr, np.float32(-np.inf))
    assert np.all(thr.astype(np.float64) > pos) and np.all(below.astype(np.float64) < pos)
    # the kernel's rule, restated: bucket = 776 + c for x >= 0, 775 - c below
    x = np.concatenate([thr, below, -thr, -below,
                        np.float32([0.0, -0.0, 1e-40, -1e-40, 3.4e38, -3.4e38, 1.0, -1.0])])
    c = np.searchsorted(thr, np.abs(x), side="right")
    got = np.where(x < 0, 775 - c, 776 + c)
    want = np.searchsorted(ref.limits(), x.astype(np.float64), side="right")
    assert np.array_equal(got, want)


# -------------------------------------------------------------- encoding ----
def _decode_histo(buf):
    out = {}
    for fn, wt, v in records._fields(buf):
        if fn <= 5:
            out[fn] = struct.unpack("<d", v)[0]
        else:
            out[fn] = np.frombuffer(v, "<f8")
    return out


@pytest.mark.parametrize("filled", [
    {0: 3},                         # a single bucket, trailing empty run
    {1550: 2},                      # leading empty run only
    {700: 1, 701: 4, 900: 2},       # leading, inner and trailing empty runs
    {0: 1, 1: 1, 1549: 1, 1550: 5},
    {},                             # all empty
    {776: 7},
])
def test_encode_histogram_runs(filled):
    counts = np.zeros(1551, np.int64)
    for k, v in filled.items():
        counts[k] = v
    num = float(counts.sum())
    h = _decode_histo(summaries.encode_histogram((-1.0, 2.0, num, 0.5, 0.25, 0.0), counts))
    want_l, want_b = ref.compress(counts)
    assert h[6].tolist() == want_l and h[7].tolist() == want_b
    assert (h[1], h[2], h[3], h[4], h[5]) == (-1.0, 2.0, num, 0.5, 0.25)
    assert h[7].sum() == num
    lim = summaries.bucket_limits()
    # every non-empty bucket is its own entry; runs carry their last limit
    assert [lim[k] for k in sorted(filled)] == [l for l, b in zip(h[6], h[7]) if b > 0]
    assert len(h[6]) <= 2 * len(filled) + 1 and h[6][-1] == lim[-1]
    if not filled:
        assert h[6].tolist() == [lim[-1]] and h[7].tolist() == [0.0]


# ------------------------------------------------------------ event file ----
def _write_events(folder):
    w = summaries.EventWriter(str(folder))
    counts = np.zeros(1551, np.int64)
    counts[[10, 776, 1200]] = [2, 5, 1]
    w.add([summaries.scalar_value("a/b_1_dig", 1.5),
           summaries.scalar_value("empty_0_dig", float("nan"))], 0)
    w.add([summaries.histogram_value("air/rnn/w", (-3.0, 4.0, 8.0, 1.0, 30.0, 0.0), counts)], 7)
    w.add([summaries.image_value("reconstruction/image/0", 2, 3, b"\x89PNGfake")], 2 ** 33)
    w.close()
    return w.path, counts


def test_event_writer_round_trip(tmp_path):
    path, counts = _write_events(tmp_path)
    assert glob.glob(str(tmp_path / "events.out.tfevents.*")) == [path]
    recs = list(records.iter_records(path, verify=True))
    assert len(recs) == 4
    first = {fn: v for fn, _, v in records._fields(recs[0])}
    assert first[3] == b"brain.Event:2" and 1 in first and 5 not in first

    def event(buf):
        ev = {fn: v for fn, _, v in records._fields(buf)}
        values = []
        for fn, _, v in records._fields(ev[5]):
            assert fn == 1
            values.append({f: x for f, _, x in records._fields(v)})
        return ev[2], values
    step, vals = event(recs[1])
    assert step == 0 and [v[1] for v in vals] == [b"a/b_1_dig", b"empty_0_dig"]
    assert struct.unpack("<f", vals[0][2])[0] == 1.5
    assert math.isnan(struct.unpack("<f", vals[1][2])[0])
    step, vals = event(recs[2])
    assert step == 7 and vals[0][1] == b"air/rnn/w"
    h = _decode_histo(vals[0][5])
    want_l, want_b = ref.compress(counts)
    assert h[6].tolist() == want_l and h[7].tolist() == want_b and h[3] == 8.0
    step, vals = event(recs[3])
    assert step == 2 ** 33
    img = {f: x for f, _, x in records._fields(vals[0][4])}
    assert (img[1], img[2], img[3], img[4]) == (2, 3, 3, b"\x89PNGfake")


def _protobuf_event_class():
    """Event and its four nested messages from the field numbers stated in
    mog_air/summaries.py, as descriptors built at test time."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="summaries_test.proto", package="t",
                                            syntax="proto3")

    def msg(name, fields):
        m = fd.message_type.add(name=name)
        for fname, num, typ, label, tname in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if tname:
                f.type_name = ".t." + tname
    O, R = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg("HistogramProto", [(n, i + 1, F.TYPE_DOUBLE, O, None) for i, n in enumerate(
        ("min", "max", "num", "sum", "sum_squares"))] + [
            ("bucket_limit", 6, F.TYPE_DOUBLE, R, None), ("bucket", 7, F.TYPE_DOUBLE, R, None)])
    msg("Image", [("height", 1, F.TYPE_INT32, O, None), ("width", 2, F.TYPE_INT32, O, None),
                  ("colorspace", 3, F.TYPE_INT32, O, None),
                  ("encoded_image_string", 4, F.TYPE_BYTES, O, None)])
    msg("Value", [("tag", 1, F.TYPE_STRING, O, None), ("simple_value", 2, F.TYPE_FLOAT, O, None),
                  ("image", 4, F.TYPE_MESSAGE, O, "Image"),
                  ("histo", 5, F.TYPE_MESSAGE, O, "HistogramProto")])
    msg("Summary", [("value", 1, F.TYPE_MESSAGE, R, "Value")])
    msg("Event", [("wall_time", 1, F.TYPE_DOUBLE, O, None), ("step", 2, F.TYPE_INT64, O, None),
                  ("file_version", 3, F.TYPE_STRING, O, None),
                  ("summary", 5, F.TYPE_MESSAGE, O, "Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("t.Event"))


def test_event_file_parses_with_protobuf(tmp_path):
    Event = _protobuf_event_class()
    path, counts = _write_events(tmp_path)
    events = []
    for rec in records.iter_records(path, verify=True):
        e = Event()
        e.ParseFromString(rec)
        events.append(e)
    assert events[0].file_version == "brain.Event:2" and events[0].wall_time > 0
    assert [e.step for e in events] == [0, 0, 7, 2 ** 33]
    assert [v.tag for v in events[1].summary.value] == ["a/b_1_dig", "empty_0_dig"]
    assert events[1].summary.value[0].simple_value == 1.5
    assert math.isnan(events[1].summary.value[1].simple_value)
    h = events[2].summary.value[0].histo
    want_l, want_b = ref.compress(counts)
    assert list(h.bucket_limit) == want_l and list(h.bucket) == want_b
    assert (h.min, h.max, h.num, h.sum, h.sum_squares) == (-3.0, 4.0, 8.0, 1.0, 30.0)
    im = events[3].summary.value[0].image
    assert (im.height, im.width, im.colorspace, im.encoded_image_string) == \
        (2, 3, 3, b"\x89PNGfake")


# ------------------------------------------------------------------ tags ----
def test_numeric_tags_are_the_references():
    tags = summaries.numeric_tags(6, 6)
    assert tags == ref.reference_tags(6, 6)
    assert len(tags) == 320 and len(set(tags)) == 320
    assert "steps_0_dig" in tags and "total_loss_all_dig" in tags
    assert "z_pres_kl_6_step_6_dig" in tags and "scale_1_step_all_dig" in tags


# -------------------------------------------------------------- refusals ----
def _args(extra):
    from mog_air import trainer
    parser = argparse.ArgumentParser()
    trainer.add_common_args(parser, reader_threads=1)
    return trainer, parser.parse_args(extra)


def test_summary_flag_defaults_and_refusals():
    trainer, args = _args([])
    assert args.summaries == 0 and args.summary_cadence == "50,250,500,100"
    assert summaries.parse_cadence(args.summary_cadence) == summaries.CADENCE
    trainer.check_summary_args(args, trainer.Dist(0, 2))  # --summaries 0: nothing to refuse
    trainer, args = _args(["--summaries", "1", "--summary-cadence", "4,8,8,4"])
    trainer.check_summary_args(args, trainer.Dist())
    with pytest.raises(ValueError, match="ranks"):
        trainer.check_summary_args(args, trainer.Dist(0, 2))
    for bad in ("4,8,8", "4,8,8,0", "a,b,c,d", "4,8,8,4,2", "", "1.5,2,3,4", "-1,2,3,4"):
        trainer, args = _args(["--summaries", "1", "--summary-cadence=" + bad])
        with pytest.raises(ValueError, match="cadence"):
            trainer.check_summary_args(args, trainer.Dist())


def test_summaries_refused_before_any_folder(tmp_path, monkeypatch):
    from mog_air import trainer
    monkeypatch.chdir(tmp_path)
    entry = __import__("training_air_original")
    monkeypatch.setattr(trainer, "distributed_setup", lambda a: trainer.Dist(0, 2))
    common = ["-dn", "13", "--iterations", "2", "-r", str(tmp_path / "res"), "-k", "x"]
    with pytest.raises(ValueError, match="ranks"):
        entry.main(common + ["--summaries", "1"])
    monkeypatch.setattr(trainer, "distributed_setup", lambda a: trainer.Dist())
    with pytest.raises(ValueError, match="cadence"):
        entry.main(common + ["--summaries", "1", "--summary-cadence", "5,5"])
    assert not glob.glob(str(tmp_path / "res*"))
