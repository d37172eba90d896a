"""omg_amd._checkpoint without a GPU and without the library: the loader, the reader and the packed-operand memo that the flat-weight
models inherit, on a toy subclass; and that the detector reads its checkpoint once."""
import json

import pytest
import torch

from omg_amd import _checkpoint as ck
from omg_amd import _lib as L


class Toy(ck.FlatWeights):
    check_config = staticmethod(dict)
    prefix = "toy."
    no_training = "'drop'"

    def shapes(self):
        return {"a.weight": (self.cfg["n"], 2), "b.bias": (3,)}

    def _pack(self):
        return {"twice": self._w["a.weight"] * 2}


def weights(n=4):
    return {"a.weight": torch.arange(2.0 * n).reshape(n, 2), "b.bias": torch.tensor([1.0, 2.0, 3.0])}


def test_keys_outside_the_prefix_are_ignored_and_the_others_are_placed():
    m = Toy({"n": 4})
    sd = {"toy." + k: v for k, v in weights().items()}
    sd.update({"other.a.weight": torch.zeros(9), "a.weight": torch.zeros(7, 7)})
    assert m.load_state_dict(sd, prefix="toy.") == ([], [])
    assert list(m.state_dict()) == ["a.weight", "b.bias"] and m.state_dict() is not m._w
    for k, v in weights().items():
        assert m._w[k].dtype == torch.float16 and torch.equal(m._w[k], v.half()), k
    # without a prefix every key is the module's own
    with pytest.raises(L.OmgHipError, match=r"Toy.load_state_dict: missing \[\], unexpected \['other.a.weight'\]"):
        Toy({"n": 4}).load_state_dict({**weights(), "other.a.weight": torch.zeros(9)})


def test_a_wrong_shape_names_the_key_and_both_shapes():
    with pytest.raises(L.OmgHipError, match=r"Toy.load_state_dict: a.weight is \(5, 2\), the config needs \(4, 2\)$"):
        Toy({"n": 4}).load_state_dict({"toy." + k: v for k, v in weights(5).items()}, prefix="toy.")


def test_missing_follows_shapes_and_long_lists_are_cut_at_six():
    m = Toy({"n": 4})
    assert m.load_state_dict({"toy.zz": torch.zeros(1), "toy.b.bias": weights()["b.bias"]}, strict=False, prefix="toy.") == (["a.weight"], ["toy.zz"])
    assert m.load_state_dict({}, strict=False) == (["a.weight", "b.bias"], [])
    with pytest.raises(L.OmgHipError, match=r"missing \['a.weight', 'b.bias'\], unexpected \['x0', 'x1', 'x2', 'x3', 'x4', 'x5'\] \.\.\.$"):
        m.load_state_dict({f"x{i}": torch.zeros(1) for i in range(7)})


def test_a_loaded_tensor_does_not_alias_the_callers():
    sd = {k: v.half() for k, v in weights().items()}          # already in the module's dtype, on its device, contiguous
    m = Toy({"n": 4})
    m.load_state_dict(sd)
    sd["b.bias"].zero_()
    assert torch.equal(m._w["b.bias"], torch.tensor([1.0, 2.0, 3.0]).half())
    assert m._w["a.weight"].data_ptr() != sd["a.weight"].data_ptr()


def test_the_pack_is_built_once_and_dropped_by_a_reload_and_a_move():
    m = Toy({"n": 4})
    assert m._packed is None
    m.load_state_dict(weights())
    pk = m._pk()
    assert m._pk() is pk and m._packed is pk and torch.equal(pk["twice"], weights()["a.weight"].half() * 2)
    m.load_state_dict({k: v + 1 for k, v in weights().items()})
    assert m._packed is None and torch.equal(m._pk()["twice"], (weights()["a.weight"] + 1).half() * 2)
    assert m.to(torch.bfloat16) is m and m._packed is None
    assert m.dtype == torch.bfloat16 and all(v.dtype == torch.bfloat16 for v in m._w.values()) and m._pk()["twice"].dtype == torch.bfloat16


def test_inference_only_and_the_storage_dtypes():
    m = Toy({"n": 4})
    assert m.eval() is m and not m.training
    with pytest.raises(L.OmgHipError, match=r"Toy: training \('drop'\) is not built; the module is inference only"):
        m.train()
    with pytest.raises(L.OmgHipError, match="^Toy: dtype torch.float32; the kernels store float16 or bfloat16"):
        Toy({"n": 4}, dtype=torch.float32)


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_from_pretrained_reads_either_file_of_a_local_directory(tmp_path, fmt):
    sd = {"toy." + k: v for k, v in weights(6).items()}
    (tmp_path / "config.json").write_text(json.dumps({"n": 6}))
    with pytest.raises(L.OmgHipError, match="Toy.from_pretrained: neither model.safetensors nor pytorch_model.bin in "):
        Toy.from_pretrained(tmp_path)
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(sd, str(tmp_path / "model.safetensors"))
    else:
        torch.save(sd, str(tmp_path / "pytorch_model.bin"))
    m = Toy.from_pretrained(tmp_path, torch_dtype=torch.bfloat16, device="cpu", some_keyword_of_the_library=True)      # the class's own prefix
    assert m.cfg == {"n": 6} and m.dtype == torch.bfloat16 and torch.equal(m._w["a.weight"], weights(6)["a.weight"].bfloat16())
    assert ck.read_checkpoint(tmp_path, "Someone")[0] == {"n": 6}
    with pytest.raises(L.OmgHipError, match="missing"):
        Toy.from_pretrained(tmp_path, prefix="")
    with pytest.raises(L.OmgHipError, match=r"Toy.from_pretrained: .*nowhere is not a local checkpoint directory with a config.json \(nothing is downloaded\)"):
        Toy.from_pretrained(tmp_path / "nowhere")


def test_the_holders_keep_the_checkpoints_names():
    w = ck.Weight((3, 2), 3, torch.float16, "cpu")
    assert [(k, tuple(v.shape), v.dtype) for k, v in w.state_dict().items()] == [("weight", (3, 2), torch.float16), ("bias", (3,), torch.float16)]
    assert list(ck.Weight((3, 2), 0, torch.float16, "cpu").state_dict()) == ["weight"] and not w.weight.requires_grad
    by_index, in_order = ck.Seq({0: w, 3: ck.Weight((1,), 0, torch.float16, "cpu")}), ck.Seq([w, ck.Weight((1,), 0, torch.float16, "cpu")])
    assert list(by_index.state_dict()) == ["0.weight", "0.bias", "3.weight"] and by_index[3] is getattr(by_index, "3")
    assert list(in_order.state_dict()) == ["0.weight", "0.bias", "1.weight"] and in_order[0] is w


def test_the_detector_reads_its_checkpoint_once(tmp_path, monkeypatch):
    from omg_amd import gdino_decoder
    from tests.test_bert import _detector_checkpoint
    sd = _detector_checkpoint(tmp_path)
    reads, read = [], ck.read_checkpoint

    def counted(path, who):
        reads.append(who)
        return read(path, who)

    monkeypatch.setattr(ck, "read_checkpoint", counted)
    monkeypatch.setattr(gdino_decoder, "read_checkpoint", counted)
    det = gdino_decoder.GroundingDinoDetector.from_pretrained(tmp_path, device="cpu", text_backbone="hip")
    assert reads == ["GroundingDinoDetector"]
    for part, key, own in ((det.backbone, "model.backbone.conv_encoder.model.swin.embeddings.norm.weight", "swin.embeddings.norm.weight"),
                           (det.text_backbone, "model.text_backbone.embeddings.LayerNorm.weight", "embeddings.LayerNorm.weight"),
                           (det.encoder, "model.level_embed", "level_embed"), (det.head, "model.enc_output.weight", "enc_output.weight")):
        assert torch.equal(part.state_dict()[own], sd[key].half()), key
    # a part on its own still reads the directory
    assert type(det.head).from_pretrained(tmp_path).cfg == det.head.cfg and reads[1:] == ["GroundingDinoDecoderHead"]
