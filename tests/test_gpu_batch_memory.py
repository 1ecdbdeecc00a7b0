"""What a batch owns and what it times, on the paths no other test walks: buffers that grow and are released inside one batch (index
tables, a window, an attached message, the batch's received stream), a second batch on the same contexts after the first is destroyed,
and every timer of pcamv_gpu_batch_kernel_time under the name include/pcamv_gpu.h lists for it.  Two CAVLC contexts of 2 x 2
macroblocks, so nothing waits for the builds of the RD instance.  The streams are the synthetic ones of tests/stream_cases.py: their
slice units are not meant to parse, only to be counted and walked.  Nothing here provokes a failure of the device or of an allocation;
the paths a failed allocation takes are checked by reading.  Run with -m gpu."""
import os
import re

import pytest

import stream_cases as stc

pytestmark = pytest.mark.gpu
W = H = 32
INDEX_KERNELS = {"k_stream_plan", "k_stream_scan", "k_stream_prefix", "k_stream_place"}


@pytest.fixture(scope="module")
def pc():
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


@pytest.fixture()
def encs(pc):
    made = []
    for _ in range(2):
        p = pc.param_default(W, H)
        pc.param_parse(p, "subme", 5)
        p.b_cabac = 0
        made.append(pc.Encoder(p))
    yield made
    for e in made:
        e.close()


def _streams():
    """(two short streams, two longer ones with more slice units, the host indexer's slice counts of each pair)"""
    by_len = sorted((s for s, _ in stc.random_streams(count=40, seed=31) if stc.host_index(s)[2]), key=len)
    short, long_ = by_len[:2], by_len[-2:]
    n_short, n_long = [stc.host_index(s)[2] for s in short], [stc.host_index(s)[2] for s in long_]
    assert max(len(s) for s in short) < min(len(s) for s in long_) and 0 < max(n_short) < min(n_long), "the second index call has to outgrow the first"
    return short, long_, n_short, n_long


def _timer_names():
    """the names the header lists at pcamv_gpu_batch_kernel_time"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pcamv_gpu.h")) as f:
        text = f.read()
    head = text[:text.index("pcamv_gpu_batch_kernel_time(")]
    names = re.findall(r'"(k_\w+)"', head[head.rindex("/*"):])
    assert len(names) == len(set(names)) == 40, names
    return names


def test_regrow_and_release_in_one_batch(pc, encs):
    short, long_, n_short, n_long = _streams()
    p = stc.params(log2_max_frame_num=9, log2_max_poc_lsb=9, deblocking_filter_control_present=1, entropy_cabac=0)
    for e in encs:
        e.rx_reserve(4000)
    b = pc.Batch(encs)
    assert b.index_streams(short, max_units=2).tolist() == n_short
    assert b.index_streams(long_, max_units=max(n_long) + 3).tolist() == n_long        # more bytes, more chunks, larger tables
    assert [v.tolist() for v in b.stream_tell()] == [[0, 0], n_long]
    b.stream_window(2)
    b.stream_window(0)
    with pytest.raises(pc.PcamvError, match="invalid argument"):       # released: there is no window to call
        b.extract_stream_window(p, 0.5, 1)
    b.stream_window(4)
    for k in (4, 3):
        b.extract_stream_window(p, 0.5, k)
        assert b.window_status().shape == (2, k)
    assert b.index_streams(short, max_units=2).tolist() == n_short      # behind a reserved window: its slots follow the index
    for n_bytes in (64, 8, 256):
        b.set_message(bytes(range(n_bytes)))
        assert b.message_tell() == (0, 8 * n_bytes)
    for n_bits in (5000, 200):
        b.rx_message_reserve(n_bits)
        assert b.rx_message_guard_intact()
        assert b.rx_message_tell()[:2] == (0, n_bits)
    b.close()
    b2 = pc.Batch(encs)
    assert b2.index_streams(short, max_units=2).tolist() == n_short
    assert b2.index_streams(long_, max_units=max(n_long) + 3).tolist() == n_long
    b2.close()


def test_every_timer_answers_to_its_name(pc, encs):
    b = pc.Batch(encs)
    names = _timer_names() + [b.dominant_kernel()]
    assert INDEX_KERNELS <= set(names)
    for name in names:
        assert b.kernel_time(name)[1] == 0, f"{name}: launches on a fresh batch"
    with pytest.raises(pc.PcamvError):
        b.kernel_time("k_no_such_kernel")
    b.index_streams(_streams()[0], max_units=2)
    launches = {name: b.kernel_time(name)[1] for name in names}
    assert launches == {name: int(name in INDEX_KERNELS) for name in names}
    b.close()
