"""The zk_raw_encoder_* / zk_encoder_* handles with a dictionary (zk_raw_encoder_set_dictionary, zk_encoder_set_dictionary,
EncodeOptions.dictionary): every policy keeps working, the setter is refused mid-frame, an explicit prefix overrides the dictionary, and the
archive with its seek table decodes through Decoder on an engine with the dictionary set.  The frames' own checks (three judges, facts) are
tests/test_gpu_encode_dict.py's; here libzstd 1.5.7 judges every frame the handles cut."""
import io

import pytest

import zeekstd_amd as zk
from zeekstd_amd import DecodeOptions, EncodeOptions, FrameSizePolicy
from zeekstd_amd import api
from helpers import dict_fixtures as df
from helpers import enc_dict_sim as S
from helpers import libzstd_dict

pytestmark = pytest.mark.gpu

DICTS = S.fixture_dicts()
TRAINED_ID = 1368370104
DATA = df.records(501, 9000)
STAGE_WRONG = -60


@pytest.fixture(scope="module")
def judge():
    j = libzstd_dict.judge()
    if j is None:
        pytest.skip("libzstd 1.5.7 is not in this image")
    yield j
    j.close()


@pytest.fixture(scope="module")
def cdict(engine):
    c = zk.EncodeDictionary(engine, zk.Dictionary(DICTS["trained"]))
    yield c
    c.close()


def frames_of(seekable, table):
    return [seekable[table.frame_start_comp(i):table.frame_end_comp(i)] for i in range(table.num_frames())]


def judged(judge, seekable, table, want, dictionary=DICTS["trained"], named=True):
    """every frame of the table decodes under libzstd 1.5.7 with the dictionary to its slice of `want`, and names it"""
    out = b""
    for f in frames_of(seekable, table):
        ff = df.frame_facts(f)
        assert ff["dict_id"] == (TRAINED_ID if named else None)
        got = judge.using_dict(f, len(want) + 64, dictionary)
        assert isinstance(got, bytes), got
        out += got
    assert out == want


def through_decoder(engine, seekable, want):
    engine.set_dictionary(zk.Dictionary(DICTS["trained"]))
    try:
        assert DecodeOptions(seekable).engine(engine).into_decoder().read_to_end() == want
    finally:
        engine.set_dictionary(None)


def raw_run(enc, data, cuts=(), out_len=97):
    """data through a RawEncoder with an output buffer of out_len bytes, end_frame after the byte counts of `cuts` and at the end"""
    buf, seekable, at = bytearray(out_len), bytearray(), 0

    def end():
        while True:
            p = enc.end_frame(buf)
            seekable.extend(buf[:p.out_progress()])
            if p.data_left() == 0:
                return
    for stop in list(cuts) + [len(data)]:
        while at < stop:
            p = enc.compress(data[at:stop], buf)
            seekable.extend(buf[:p.out_progress()])
            at += p.in_progress()
        end()
    return bytes(seekable)


@pytest.mark.parametrize("policy", [FrameSizePolicy.Uncompressed(1024), FrameSizePolicy.Compressed(300)], ids=["uncompressed1024", "compressed300"])
@pytest.mark.parametrize("out_len", [1, 97])
def test_raw_encoder_with_a_dictionary(engine, judge, cdict, policy, out_len):
    """end_frame after 0, 1 and 700 bytes and at the end; output buffers of one byte"""
    enc = EncodeOptions().engine(engine).frame_size_policy(policy).checksum_flag(True).dictionary(cdict).into_raw_encoder()
    seekable = raw_run(enc, DATA, cuts=(0, 1, 701), out_len=out_len)
    st = enc.seek_table()
    assert st.size_comp() == len(seekable) and st.size_decomp() == len(DATA)
    assert st.frame_size_decomp(0) == 0 and st.frame_size_decomp(1) == 1 and st.frame_size_decomp(2) == 700
    judged(judge, seekable, st, DATA)
    ser, tail, buf = st.into_serializer(), bytearray(), bytearray(64)
    while True:
        n = ser.write_into(buf)
        if n == 0:
            break
        tail += buf[:n]
    through_decoder(engine, seekable + bytes(tail), DATA)


def test_setter_mid_frame_is_refused_and_changes_nothing(engine, judge, cdict):
    enc = EncodeOptions().engine(engine).frame_size_policy(FrameSizePolicy.Uncompressed(4096)).into_raw_encoder()
    buf = bytearray(1 << 16)
    enc.compress(DATA[:100], buf)
    with pytest.raises(api.Error) as ex:
        enc.set_dictionary(cdict)
    assert ex.value.code == STAGE_WRONG
    seekable = raw_run(enc, DATA[100:3000], out_len=4096)
    st = enc.seek_table()
    judged(judge, seekable, st, DATA[:3000], dictionary=None, named=False)        # still no dictionary
    enc.set_dictionary(cdict)                                                     # between frames it is allowed
    more = raw_run(enc, DATA[3000:5000], out_len=4096)
    f = more
    assert df.frame_facts(f)["dict_id"] == TRAINED_ID and judge.using_dict(f, 4096, DICTS["trained"]) == DATA[3000:5000]
    enc.compress(DATA[:10], buf)
    with pytest.raises(api.Error) as ex:
        enc.set_dictionary(None)
    assert ex.value.code == STAGE_WRONG
    f = raw_run(enc, b"", out_len=4096)
    assert df.frame_facts(f)["dict_id"] == TRAINED_ID                             # the refused call changed nothing
    enc.set_dictionary(None)
    f = raw_run(enc, DATA[:500], out_len=4096)
    assert df.frame_facts(f)["dict_id"] is None


def test_an_explicit_prefix_overrides_the_dictionary(engine, judge, cdict):
    prefix = df.records(502, 3000)
    enc = EncodeOptions().engine(engine).frame_size_policy(FrameSizePolicy.Uncompressed(2000)).dictionary(cdict).into_raw_encoder()
    buf = bytearray(1 << 16)
    p = enc.compress_with_prefix(DATA[:2000], buf, prefix)
    assert p.in_progress() == 2000
    a = raw_run(enc, b"", out_len=4096)                                           # the frame begun under the prefix
    b = raw_run(enc, DATA[2000:4000], out_len=4096)                               # the next one: the dictionary again
    assert df.frame_facts(a)["dict_id"] is None and df.frame_facts(b)["dict_id"] == TRAINED_ID
    want, _ = engine.encode_frames(DATA[:2000], 2000, 0, False, prefix=prefix)
    assert a == want
    assert judge.using_dict(b, 4096, DICTS["trained"]) == DATA[2000:4000]


@pytest.mark.parametrize("policy", [FrameSizePolicy.Uncompressed(1024), FrameSizePolicy.Compressed(300)], ids=["uncompressed1024", "compressed300"])
def test_encoder_with_a_dictionary(engine, judge, cdict, policy):
    sink = io.BytesIO()
    enc = EncodeOptions().engine(engine).frame_size_policy(policy).dictionary(cdict).into_encoder(sink)
    enc.end_frame()                                                               # after 0 bytes: an empty frame
    enc.compress(DATA[:1]); enc.end_frame()
    enc.compress(DATA[1:701])
    with pytest.raises(api.Error) as ex:                                          # a frame is open
        enc.set_dictionary(None)
    assert ex.value.code == STAGE_WRONG
    enc.end_frame()
    for at in range(701, len(DATA), 1500):
        enc.compress(DATA[at:at + 1500])
    enc.finish()
    seekable = sink.getvalue()
    table = zk.SeekTable.from_seekable(seekable)
    through_decoder(engine, seekable, DATA)
    assert table.frame_size_decomp(0) == 0 and table.frame_size_decomp(1) == 1 and table.frame_size_decomp(2) == 700
    judged(judge, seekable, table, DATA)


def test_encoder_equals_level_a_under_uncompressed(engine, cdict):
    """the frames an Encoder cuts under Uncompressed(n) are zk_encode_frames_dict's"""
    sink = io.BytesIO()
    enc = EncodeOptions().engine(engine).frame_size_policy(FrameSizePolicy.Uncompressed(1000)).compression_level(1).checksum_flag(True).dictionary(cdict).into_encoder(sink)
    enc.compress(DATA)
    enc.end_frame()
    want, pairs = engine.encode_frames(DATA, 1000, 1, True, dictionary=cdict)
    enc.finish()
    assert sink.getvalue()[:len(want)] == want
