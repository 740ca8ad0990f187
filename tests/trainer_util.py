"""The two tiny-trainer builders the suite shares."""
from conftest import pkg


def cpu_trainer(**kw):
    """W2V2_TINY modules with their constructors' own weights on the CPU: for what the constructor resolves, checks and refuses."""
    init = pkg("utils.init"); enc = pkg("model.encoder"); fm = pkg("model.fusion_module"); dm = pkg("model.decoder")
    tr = pkg("model.trainer"); tok = pkg("utils.tokenizer")
    cfg = dict(init.W2V2_TINY)
    return tr.MultimodalTrainer(enc.VisualEncoder(), enc.AudioEncoder(cfg, freeze=True), fm.CrossAttentionFusion(512, cfg["hidden_size"], 512),
                                dm.CTCDecoder(1024, 800, 3), tok.SyntheticTokenizer(800), device="cpu", **kw)


def gpu_trainer(cfg, precision, **kw):
    """The seeded utils.init weights on the GPU with main.py's freeze policy and the fixed projection; ``kw`` goes to the constructor."""
    init = pkg("utils.init"); enc = pkg("model.encoder"); fm = pkg("model.fusion_module"); dm = pkg("model.decoder")
    tr = pkg("model.trainer"); tok = pkg("utils.tokenizer")
    pkg("precision").set_precision(precision)
    ve = enc.VisualEncoder(); ve.load_state_dict(init.visual_state_dict())
    for p in ve.parameters():
        p.requires_grad = False                                        # main.py:100-103
    ae = enc.AudioEncoder(dict(cfg), freeze=True); ae.load_state_dict(init.w2v2_state_dict(cfg))
    for n, p in ae.model.named_parameters():                           # main.py:26-31
        p.requires_grad = any(f"encoder.layers.{i}." in n for i in range(6, 10))
    fu = fm.CrossAttentionFusion(512, cfg["hidden_size"], 512); fu.load_state_dict(init.fusion_state_dict(512, cfg["hidden_size"], 512))
    de = dm.CTCDecoder(1024, 800, 3); de.load_state_dict(init.decoder_state_dict(1024, 800))
    t = tr.MultimodalTrainer(ve, ae, fu, de, tok.SyntheticTokenizer(800), **{"learning_rate": 1e-4, "device": "cuda", "lambda_": 0.1, **kw})
    t.fixed_projection = init.projection_params(cfg["hidden_size"])
    return t
