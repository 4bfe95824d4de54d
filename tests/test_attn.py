"""SelfAttention of ops/attn.py and PyBiLstmAttn / PyBiLstmAttnCrf on the torch path (CPU)."""
import pytest
import torch


def test_self_attention_reads_no_padded_position_and_keeps_an_empty_sentence():
    from rafiki_amd.ops.attn import SelfAttention
    torch.manual_seed(0)
    att = SelfAttention(12, 2, 5).double()
    lens = torch.tensor([6, 3, 0])
    live = torch.arange(6)[None] < lens[:, None]
    h = torch.randn(3, 6, 12, dtype=torch.float64)
    g = torch.where(live[..., None], h, torch.full_like(h, 1e3)).requires_grad_(True)   # garbage past the lengths
    out = att(g, lens)
    assert torch.equal(out[live], att(h, lens)[live])
    assert torch.equal(out[2], g[2])                                                    # the empty sentence
    out.square().sum().backward()
    assert torch.isfinite(g.grad).all() and all(torch.isfinite(p.grad).all() for p in att.parameters())


@pytest.mark.parametrize('name', ['PyBiLstmAttn', 'PyBiLstmAttnCrf'])
def test_pybilstmattn_cpu_trains_predicts_and_reloads(name):
    from rafiki_amd.models import ZOO, pos_tagging
    from rafiki_amd.ops.attn import SelfAttention
    cls = getattr(pos_tagging, name)
    knobs = dict(epochs=2, word_embed_dims=16, word_rnn_hidden_size=16, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32, clip_norm=1.0, attn_heads=2, attn_head_dims=9)
    m = cls(**knobs)
    m.train("synthetic://corpus?n=200&seed=0")
    assert isinstance(m._net.attn, SelfAttention) and hasattr(m._net, 'crf') == name.endswith('Crf')
    queries = [["a", "b", "c"], ["d"], ["e", "f", "g", "h", "i"]]
    out = m.predict(queries)
    assert [len(o) for o in out] == [3, 1, 5] and all(0 <= t < m._tag_count for o in out for t in o)
    m2 = cls(**knobs)
    m2.load_parameters(m.dump_parameters())
    assert m2.predict(queries) == out
    assert ZOO[name] == ('pos_tagging.py', 'POS_TAGGING') and {'attn_heads', 'attn_head_dims'} <= set(cls.get_knob_config())
