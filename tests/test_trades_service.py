"""The service's trade stream (me_service_trades_subscribe / me_service_trades_stream) where no engine is
needed: a matcher-backed service has no trade feed, and streaming needs a subscription. Runs on CPU."""
import ctypes as C

import pytest

from tests.service_common import FeedMatcher


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def test_a_matcher_has_no_trade_feed(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=FeedMatcher(1))
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.trades_subscribe()
        assert ei.value.code == me.ME_E_INVALID and "no trade feed" in str(ei.value)
        svc.trades_subscribe(False)  # turning an absent stream off is not an error
    finally:
        svc.close()


def test_streaming_needs_a_subscription(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=FeedMatcher(1))
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.trades_stream()
        assert ei.value.code == me.ME_E_INVALID and "not subscribed" in str(ei.value)
        with pytest.raises(me.ServiceError):
            svc.trades_stream("A")
    finally:
        svc.close()


def test_entry_points_are_exported_and_refuse_null(built):
    from matching_engine_amd import _abi

    assert C.sizeof(_abi.MeTradeUpdate) == 104
    lib = _abi.load()
    for name in ("me_service_trades_subscribe", "me_service_trades_stream"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    assert lib.me_service_trades_subscribe(None, 1) == _abi.ME_E_INVALID
    assert lib.me_service_trades_stream(None, None, None, 0, None) == _abi.ME_E_INVALID
