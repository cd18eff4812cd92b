"""config.use_fused_seg_tail: the fused replicated tail is taken by size unless the switch forces it either way (no GPU needed)."""
from yolo_dual_amd import config


def test_switch_states():
    was = config.fused_seg_tail()
    try:
        config.set_fused_seg_tail(None)
        assert config.SEG_TAIL_MIN_PIXELS == 262144
        assert not config.use_fused_seg_tail(2 * 16 * 16)             # the 2 x 64^2 steps of the suite
        assert not config.use_fused_seg_tail(8 * 128 * 128)           # the largest recorded launch trace
        assert not config.use_fused_seg_tail(262143)
        assert config.use_fused_seg_tail(262144)
        assert config.use_fused_seg_tail(16 * 160 * 160)              # the flagship step
        config.set_fused_seg_tail(True)
        assert config.fused_seg_tail() is True and config.use_fused_seg_tail(1)
        config.set_fused_seg_tail(False)
        assert config.fused_seg_tail() is False and not config.use_fused_seg_tail(1 << 30)
    finally:
        config.set_fused_seg_tail(was)
