"""The two heads run side by side (engine.hip: the heads' first convs as one stage, the policy head's output tiles after
the value head's in one buffer and past its fourth tile in the strip, net_dev.hpp).  Every network width the fused
program accepts, with both value-head activations, against the float32 reference network: a tile written to or read
from the wrong slots shows up here as a wrong logit or value."""
import numpy as np
import pytest

WIDTHS = list(range(4, 65, 4))      # nz_engine_set_weights: multiples of 4 in (0, 64]; policy_channels is always 1


def _positions():
    from oracle import ttt as ottt
    codes = ottt.reachable_positions()[::9]
    x = np.zeros((len(codes), 2, 3, 3), np.float32)
    for i, c in enumerate(codes):
        g = ottt.TicTacToe()
        g.board = ottt.board_from_code(c)
        x[i] = g.state_image()[0]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("value_activation", ["tanh", "relu"])
def test_head_stages_match_reference(value_activation):
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    from nuzero_amd.weights import synthetic_recurrent_net_weights
    from oracle.net import RecurrentNetRef

    x = _positions()
    eng = SelfPlayEngine(legacy_ttt_search_config(), 16)
    for width in WIDTHS:
        w = synthetic_recurrent_net_weights(width, 2, 1, width, 2, True, 2.0)
        eng.set_weights(w, width=width, value_activation=value_activation, recurrent_iterations=2)
        logits, value, _ = eng.net_forward(x, want_probs=False)
        logits, value = logits.cpu().numpy(), value.cpu().numpy()
        p_ref, v_ref = RecurrentNetRef(w, 2, 1, width, 2, True, value_activation).inference(x, 2)
        p_ref, v_ref = p_ref.reshape(len(x), 9), v_ref.reshape(-1)
        scale = max(1.0, float(np.abs(p_ref).max()))
        assert np.abs(logits - p_ref).max() <= 1e-5 * scale, (width, value_activation)
        assert np.abs(value - v_ref).max() <= 1e-5, (width, value_activation)
    eng.close()
