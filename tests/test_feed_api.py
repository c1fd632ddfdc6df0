"""The change feed's entry points at the C-ABI boundary, without a device:
each refuses null arguments with RF_EINVAL and a message in rf_last_error
before touching one, and the bindings carry the header's constants."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "reflow_hip.h")


@pytest.fixture(scope="module")
def L():
    from reflow_amd import capi
    return capi.lib()


def refused(L, rc):
    from reflow_amd import capi
    assert rc == capi.RF_EINVAL
    assert len(L.rf_last_error()) > 0


def test_feed_entry_points_refuse_null_arguments(L):
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    refused(L, L.rf_graph_feed_open(None, None))
    refused(L, L.rf_graph_feed_open(None, p))
    refused(L, L.rf_graph_feed_close(None))
    refused(L, L.rf_graph_feed_stats_get(None, None))
    refused(L, L.rf_graph_feed_stats_get(None, p))
    # the host poll: graph, found and written always; slots and digests when cap > 0
    refused(L, L.rf_graph_feed_poll(None, 0, 0, None, None, p, p))
    refused(L, L.rf_graph_feed_poll(None, 0, 4, p, p, p, p))
    # the device poll: graph and d_n2 always
    refused(L, L.rf_graph_feed_poll_device(None, 0, 0, None, None, p, None))
    refused(L, L.rf_graph_feed_poll_device(None, 0, 4, p, p, p, None))
    # the fused lookup: graph and assoc always (the liveset may be null)
    refused(L, L.rf_graph_feed_lookup_device(None, None, None, 0, 0, 0, None, None, None, None, p, None))
    refused(L, L.rf_graph_feed_lookup_device(None, None, None, 0, 0, 4, p, p, p, p, p, None))


def test_feed_constants_match_the_header():
    from reflow_amd import capi
    text = open(HEADER).read()
    assert int(re.search(r"#define RF_FEED_FORCE_SCAN (\d+)u", text).group(1)) == capi.RF_FEED_FORCE_SCAN
    m = re.search(r"enum \{ RF_FEED_NONE = (\d+), RF_FEED_LISTED = (\d+), RF_FEED_SCAN = (\d+) \};", text)
    assert tuple(map(int, m.groups())) == (capi.RF_FEED_NONE, capi.RF_FEED_LISTED, capi.RF_FEED_SCAN)
    # the tile the header's footprint note and the GPU tests' edge sizes use
    assert capi.FEED_TILE_SLOTS == 8192 and "padded to 8192 slots" in text
    assert ctypes.sizeof(capi.GraphFeedStats) == 48
    for name in ("feed_open", "feed_close", "feed_poll", "feed_poll_device", "feed_lookup_device", "feed_stats"):
        assert callable(getattr(capi.Graph, name))
