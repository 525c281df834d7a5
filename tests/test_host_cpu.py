"""Host-side logic of the drop-in (CPU only): input contract, processor, parser plumbing, weights IO,
page sharding and the result gather (gloo, world_size 2)."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from dots_ocr_amd import dp
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.image_utils import fetch_image, preprocess_image, smart_resize, to_rgb
from dots_ocr_amd.processing import IMG_PAD, DotsOcrProcessor, process_vision_info
from dots_ocr_amd.synthetic import A4_200DPI, synth_page, synth_prompt_ids
from dots_ocr_amd.weights import expected_tensors, load_state_dict, random_state_dict, save_safetensors

GOLD = Path(__file__).parent / "golden"
ROOT = Path(__file__).resolve().parent.parent


def test_smart_resize_matches_reference_golden():
    for c in json.loads((GOLD / "smart_resize.json").read_text()):
        try:
            got = list(smart_resize(c["h"], c["w"], 28, c["min_pixels"], c["max_pixels"]))
        except ValueError:
            got = "ValueError"
        assert got == c["out"], c


def test_prompts_are_byte_identical_to_reference():
    # golden/prompts.json is the reference's dict_promptmode_to_prompt as written out by golden/make_golden.py
    from dots_ocr_amd.prompts import dict_promptmode_to_prompt
    gold = json.loads((GOLD / "prompts.json").read_text(encoding="utf-8"))
    assert len(gold) == 8
    assert dict_promptmode_to_prompt == gold


def test_preprocess_matches_oracle_and_a4_geometry():
    from oracle import image_processor as oip
    rng = np.random.default_rng(1)
    for (w, h) in [(333, 517), (100, 40), (28, 28)]:
        img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB")
        a, ga = preprocess_image(img)
        b, gb = oip.preprocess(img)
        assert list(ga) == list(gb) and np.array_equal(a, b)
    pv, thw = preprocess_image(synth_page(0, A4_200DPI))
    assert thw == [1, 168, 118] and pv.shape == (19824, 588)      # A4@200dpi -> 19 824 patches


def test_rgba_is_composited_on_white():
    im = Image.new("RGBA", (4, 4), (0, 0, 0, 0))
    assert to_rgb(im).getpixel((0, 0)) == (255, 255, 255)
    assert fetch_image(im).mode == "RGB"
    assert fetch_image(Image.new("RGB", (100, 50)), min_pixels=3136, max_pixels=11289600).size == (112, 56)


def test_processor_hf_call_surface():
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    page = synth_page(1, (140, 84))
    msgs = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": "héllo"}]}]
    text = proc.apply_chat_template(msgs, tokenize=False, add_generation_prompt=True)
    assert text == "<|user|><|img|><|imgpad|><|endofimg|>héllo<|endofuser|><|assistant|>"
    imgs, vids = process_vision_info(msgs)
    assert vids is None and len(imgs) == 1
    inputs = proc(text=[text, text], images=imgs * 2, padding=True, return_tensors="pt")
    gh, gw = inputs.image_grid_thw[0, 1].item(), inputs.image_grid_thw[0, 2].item()
    assert (inputs.input_ids[0] == cfg.image_token_id).sum().item() == gh * gw // 4
    assert inputs.pixel_values.shape == (2 * gh * gw, cfg.vision.patch_dim)
    assert inputs.attention_mask.all()
    new = proc.tokenizer.encode("héllo wörld") + [cfg.eos_token_ids[0]]
    assert proc.batch_decode([torch.tensor(new)], skip_special_tokens=True, clean_up_tokenization_spaces=False) == ["héllo wörld"]
    with pytest.raises(ValueError):
        proc(text=[text], images=[], return_tensors="pt")
    # ragged batch -> left padding, mask marks the real tokens
    short = proc.apply_chat_template([{"role": "user", "content": "hi"}])
    both = proc(text=[text, short], images=imgs, return_tensors="pt")
    assert both.attention_mask[1].sum().item() == len(proc.tokenizer.encode(short)) and both.attention_mask[1, 0].item() == 0


class _FakeModel:
    """Stands in for the engine: returns a canned layout JSON as token ids (CPU test of the parser plumbing)."""

    def __init__(self, proc, text):
        self.proc, self.text, self.calls = proc, text, []

    def generate(self, input_ids=None, max_new_tokens=0, **kw):
        self.calls.append(input_ids.shape[0])
        new = torch.tensor(self.proc.tokenizer.encode(self.text))
        return torch.cat([input_ids, new.unsqueeze(0).expand(input_ids.shape[0], -1)], dim=1)


def test_parser_plumbing_writes_reference_outputs(tmp_path):
    from dots_ocr.parser import DotsOCRParser
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    cells = [{"bbox": [28, 28, 140, 56], "category": "Title", "text": "# Hello"},
             {"bbox": [28, 84, 280, 112], "category": "Page-footer", "text": "p. 1"}]
    model = _FakeModel(proc, json.dumps(cells))
    parser = DotsOCRParser(model=model, processor=proc, output_dir=str(tmp_path))
    img_path = tmp_path / "page.png"
    synth_page(0, (600, 400)).save(img_path)
    res = parser.parse_file(str(img_path), prompt_mode="prompt_layout_all_en")
    assert len(res) == 1 and res[0]["page_no"] == 0 and res[0]["file_path"] == str(img_path)
    ih, iw = smart_resize(400, 600)
    assert (res[0]["input_height"], res[0]["input_width"]) == (ih, iw)
    out = json.loads(Path(res[0]["layout_info_path"]).read_text())
    sx, sy = iw / 600, ih / 400
    assert out[0]["bbox"] == [int(28 / sx), int(28 / sy), int(140 / sx), int(56 / sy)]          # model space -> original
    assert Path(res[0]["md_content_path"]).read_text() == "# Hello\n\np. 1"
    assert Path(res[0]["md_content_nohf_path"]).read_text() == "# Hello"
    assert (tmp_path / "page.jsonl").exists() and Path(res[0]["layout_image_path"]).exists()
    # malformed generation -> OutputCleaner salvage, filtered flag set (reference parser.py:187-207, layout_utils.py:221-228):
    # nothing recoverable in "not json" -> empty markdown; a page cut off mid-cell keeps the text of its complete cells
    parser.model = _FakeModel(proc, "not json")
    bad = parser.parse_file(str(img_path), prompt_mode="prompt_layout_all_en")[0]
    assert bad["filtered"] is True and Path(bad["md_content_path"]).read_text() == ""
    parser.model = _FakeModel(proc, json.dumps(cells)[:-30])
    cut = parser.parse_file(str(img_path), prompt_mode="prompt_layout_all_en")[0]
    assert cut["filtered"] is True and Path(cut["md_content_path"]).read_text() == "# Hello"
    # plain-text mode
    parser.model = _FakeModel(proc, "some text")
    txt = parser.parse_file(str(img_path), prompt_mode="prompt_ocr")[0]
    assert Path(txt["md_content_path"]).read_text() == "some text"
    # all pages of a document go through ONE batched generate
    parser.model = _FakeModel(proc, json.dumps(cells))
    pages = [synth_page(i, (300, 200)) for i in range(3)]
    rs = parser.parse_pages(pages, "doc", "prompt_layout_all_en", str(tmp_path))
    assert parser.model.calls == [3] and [r["page_no"] for r in rs] == [0, 1, 2]
    with pytest.raises(ValueError):
        parser.parse_file(str(tmp_path / "x.txt"))


def test_weights_inventory_and_safetensors_roundtrip(tmp_path):
    cfg = DotsConfig.tiny()
    sd = random_state_dict(cfg, seed=3)
    assert set(sd) == set(expected_tensors(cfg)) and all(tuple(sd[k].shape) == s for k, s in expected_tensors(cfg).items())
    assert torch.equal(random_state_dict(cfg, seed=3, threads=4)["lm_head.weight"], sd["lm_head.weight"])
    save_safetensors(sd, tmp_path / "model.safetensors")
    back = load_state_dict(tmp_path)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    full = DotsConfig()
    assert full.lm_param_count() == 1_777_088_000                      # SURVEY §0.3 cross-check
    n_vis = sum(int(np.prod(s)) for k, s in expected_tensors(full).items() if k.startswith("vision_tower."))
    assert abs(n_vis - 1.262e9) < 5e6


def test_config_from_pretrained(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps({
        "hidden_size": 1536, "num_hidden_layers": 28, "num_attention_heads": 12, "num_key_value_heads": 2,
        "intermediate_size": 8960, "vocab_size": 151936, "rope_theta": 1000000, "rms_norm_eps": 1e-6,
        "image_token_id": 151665, "vision_config": {"embed_dim": 1536, "num_hidden_layers": 42, "num_attention_heads": 12,
                                                     "intermediate_size": 4224, "patch_size": 14, "spatial_merge_size": 2}}))
    (tmp_path / "generation_config.json").write_text(json.dumps({"eos_token_id": [151643, 151673]}))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"min_pixels": 3136, "max_pixels": 11289600}))
    cfg = DotsConfig.from_pretrained(tmp_path)
    assert cfg.head_dim == 128 and cfg.eos_token_ids == (151643, 151673) and cfg.vision.head_dim == 128
    assert cfg.to_dict() == DotsConfig().to_dict()


def test_shard_pages_lpt():
    costs = [dp.page_cost(n) for n in [19824] * 5 + [1440, 1440, 57600, 5032, 9216]]
    bins = dp.shard_pages(costs, 4)
    assert sorted(i for b in bins for i in b) == list(range(10))
    loads = [sum(costs[i] for i in b) for b in bins]
    assert max(loads) <= max(costs) + 1e-9 or max(loads) / (sum(costs) / 4) < 1.6
    assert dp.shard_pages([1.0] * 8, 8) == [[i] for i in range(8)]
    ids, lens = np.arange(12).reshape(3, 4), np.array([4, 2, 0])
    assert dp.gather_token_ids(ids, lens) == [(0, [0, 1, 2, 3]), (1, [4, 5]), (2, [])]


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dots_ocr_amd import dp as _dp
    pages = _dp.shard_pages([3.0, 1.0, 2.0, 2.5, 0.5], world)[rank]
    n = len(pages)
    out = np.zeros((n, 6), np.int32)
    lens = np.zeros((n,), np.int32)
    for j, p in enumerate(pages):
        lens[j] = p + 1
        out[j, : p + 1] = np.arange(p + 1) + 100 * p
    res = _dp.gather_token_ids(out, lens, page_index=pages)
    q.put((rank, res))
    dist.destroy_process_group()


def test_result_gather_world_size_2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [(p, (np.arange(p + 1) + 100 * p).tolist()) for p in range(5)]
    assert got[0] == want and got[1] == want            # every rank sees the whole job, page order restored


def test_synthetic_prompt_shape():
    cfg = DotsConfig()
    ids = synth_prompt_ids(cfg, 4956)
    assert len(ids) == 5200 and int((ids == cfg.image_token_id).sum()) == 4956


def test_bicubic_tables_match_oracle():
    from dots_ocr_amd.image_utils import bicubic_resample_tables
    from oracle.image_processor import pil_bicubic_coeffs
    for (i, o) in [(1654, 1652), (2339, 2352), (100, 112), (50, 28), (36, 28), (3000, 28), (28, 700), (583, 588)]:
        k1, b1 = pil_bicubic_coeffs(i, o)
        k2, b2 = bicubic_resample_tables(i, o)
        assert np.array_equal(k1, k2) and np.array_equal(b1, b2), (i, o)


def test_plan_batches_respects_sequence_and_patch_budgets():
    from dots_ocr_amd.modeling import plan_batches
    assert plan_batches([19824] * 8, 8, 8 * 19824 + 64) == [list(range(8))]
    assert plan_batches([57600] * 3, 8, 158656) == [[0, 1], [2]]                  # max-res pages: patch budget splits the batch
    assert plan_batches([10] * 5, 2, 1000) == [[0, 1], [2, 3], [4]]
    assert plan_batches([0, 0, 0], 8, 100) == [[0, 1, 2]]                           # text-only prompts
    with pytest.raises(ValueError):
        plan_batches([200], 8, 100)


def test_continuous_batcher_admission_and_refill_with_a_fake_engine():
    """Scheduler logic only (no GPU): FIFO admission within the patch / token budgets, lowest free slot first, refill on finish."""
    import numpy as np
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request

    from fakes import FakeSlotEngine
    eng = FakeSlotEngine(lambda prompt: int(prompt[0]) + np.arange(200))       # "tokens" identify the request
    cb = ContinuousBatcher(eng, eos_ids=(7,), chunk=4)
    assert eng.eos == [7]
    def req(first, n_tok, cap, patches=0):
        ids = np.full(n_tok, first, np.int32)
        if patches:
            return Request(ids, np.zeros((patches, 4), np.float32), np.array([[1, patches // 2, 2]]), cap)
        return Request(ids, None, None, cap)
    reqs = [req(10, 20, 9, 40), req(20, 20, 1, 40), req(30, 20, 6, 40),      # third does not fit the 100-patch ViT budget with the first two
            req(40, 50, 3), req(50, 30, 200), req(60, 10, 5)]                # 50 + 30 tokens exceed the 64-token prefill budget
    out = cb.run(reqs)
    assert [o.tolist() for o in out] == [list(range(r.input_ids[0], r.input_ids[0] + min(r.max_new_tokens, 128 - len(r.input_ids))))
                                         for r in reqs]
    assert len(out[4]) == 98                                                 # cap clamped to the context capacity
    pre = [e[1] for e in eng.log if e[0] == "prefill"]
    assert pre[0] == (0, 1)                                                  # two pages fit the ViT budget
    assert pre[1] == (1,)                                                    # request 1 finished at prefill: its slot is reused at once
    assert all(len(p) <= 3 for p in pre) and sum(len(p) for p in pre) == 6
    vit = [e for e in eng.log if e[0] == "vit"]
    assert [v[1] for v in vit] == [80, 40] and [v[2] for v in vit] == [80, 40]
    assert cb.idle and not eng.slots
    with pytest.raises(ValueError):
        cb.submit(req(1, 200, 4))                                            # longer than max_seq_len
    with pytest.raises(ValueError):
        cb.submit(req(1, 10, 4, 400))                                        # more patches than the ViT workspace


def test_parse_pages_pipeline_over_engine_slots(tmp_path):
    """DotsOCRParser.parse_pages with a model that has engine slots (stand-in engine): pages are prepared on host threads,
    admitted in order into 3 slots, finished pages are post-processed on host threads; outputs equal the one-page path."""
    from dots_ocr.parser import DotsOCRParser
    from fakes import FakeSlotEngine
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)

    class SlotModel:
        config = cfg

        def __init__(self):
            def script(prompt):
                n_img = int((prompt == cfg.image_token_id).sum())
                cells = [{"bbox": [28, 28, 140, 56], "category": "Title", "text": f"# page with {n_img} vision tokens"}]
                return proc.tokenizer.encode(json.dumps(cells)) + [cfg.eos_token_ids[0]]
            self.engine = FakeSlotEngine(script, max_batch=3, max_patches=1 << 20, max_prefill_tokens=1 << 20, max_seq_len=1 << 16)
            self.engine.set_sampling(0.7, 0.9, 1)

    model = SlotModel()
    parser = DotsOCRParser(model=model, processor=proc, output_dir=str(tmp_path), num_thread=4)
    sizes = [(300, 200), (420, 280), (280, 280), (560, 420), (300, 200), (336, 504), (200, 300)]
    pages = [synth_page(i, s) for i, s in enumerate(sizes)]
    rs = parser.parse_pages(pages, "doc", "prompt_layout_all_en", str(tmp_path), input_path="doc.pdf")
    assert [r["page_no"] for r in rs] == list(range(7)) and all(r["file_path"] == "doc.pdf" for r in rs)
    assert model.engine.sampling[0] == 0.0                                       # greedy, like the reference's HF path
    for r, (w, h) in zip(rs, sizes):
        ih, iw = smart_resize(h, w)
        assert (r["input_height"], r["input_width"]) == (ih, iw)
        md = Path(r["md_content_path"]).read_text()
        assert md == f"# page with {(ih // 14) * (iw // 14) // 4} vision tokens"
        assert Path(r["layout_info_path"]).exists() and Path(r["layout_image_path"]).exists()
    pre = [e[1] for e in model.engine.log if e[0] == "prefill"]
    assert sum(len(p) for p in pre) == 7 and all(len(p) <= 3 for p in pre) and not model.engine.slots


def test_generation_config_defaults_follow_hf_semantics():
    from dots_ocr_amd.modeling import resolve_sampling
    assert resolve_sampling({}) == (0.0, 1.0)                                            # no config: greedy
    assert resolve_sampling({"do_sample": True, "temperature": 0.7, "top_p": 0.8}) == (0.7, 0.8)   # checkpoint default
    assert resolve_sampling({"do_sample": True, "temperature": 0.7}, do_sample=False) == (0.0, 1.0)  # explicit argument wins
    assert resolve_sampling({"do_sample": False}, do_sample=True, temperature=0.5) == (0.5, 1.0)
    assert resolve_sampling({"do_sample": True, "temperature": 0.0}) == (0.0, 1.0)
    assert resolve_sampling({}, do_sample=True, temperature=1.0, top_p=3.0) == (1.0, 1.0)


def test_checkpoint_chat_template_is_rendered_like_transformers(tmp_path):
    """When the checkpoint ships a Jinja chat template the processor renders it (as AutoProcessor.apply_chat_template does,
    parser.py:93-97) instead of the built-in dots.ocr format; the two agree on the reference's message shape."""
    from dots_ocr_amd.processing import load_chat_template
    cfg = DotsConfig.tiny()
    tmpl = ("{%- for m in messages %}{%- if m['role'] == 'system' %}{{ m['content'] }}{%- else %}"
            "{{ '<|' + m['role'] + '|>' }}{%- if m['content'] is string %}{{ m['content'] }}{%- else %}"
            "{%- for c in m['content'] %}{%- if c['type'] == 'image' %}{{ '<|img|><|imgpad|><|endofimg|>' }}"
            "{%- elif c['type'] == 'text' %}{{ c['text'] }}{%- endif %}{%- endfor %}{%- endif %}"
            "{{ '<|endof' + m['role'] + '|>' }}{%- endif %}{%- endfor %}"
            "{%- if add_generation_prompt %}{{ '<|assistant|>' }}{%- endif %}")
    (tmp_path / "chat_template.json").write_text(json.dumps({"chat_template": tmpl}))
    assert load_chat_template(tmp_path) == tmpl
    assert load_chat_template(tmp_path / "nope") is None
    msgs = [{"role": "user", "content": [{"type": "image", "image": "x.png"}, {"type": "text", "text": "Parse this."}]}]
    builtin = DotsOcrProcessor(cfg)
    templated = DotsOcrProcessor(cfg, chat_template=tmpl)
    want = "<|user|><|img|><|imgpad|><|endofimg|>Parse this.<|endofuser|><|assistant|>"
    assert builtin.apply_chat_template(msgs, tokenize=False, add_generation_prompt=True) == want
    assert templated.apply_chat_template(msgs, tokenize=False, add_generation_prompt=True) == want
    assert templated.apply_chat_template(msgs, tokenize=False, add_generation_prompt=False) == want[:-len("<|assistant|>")]
    assert templated.apply_chat_template(msgs, tokenize=True) == builtin.tokenizer.encode(want)
    bad = DotsOcrProcessor(cfg, chat_template="{{ raise_exception('no system role') }}")
    with pytest.raises(ValueError, match="no system role"):
        bad.apply_chat_template(msgs)


def _dp_job_pages():
    """A mixed job (BASELINE config 4 geometry in miniature): (first prompt token, prompt length, patches, cap)."""
    rng = np.random.default_rng(2025)
    return [(int(10 + i), int(rng.integers(8, 40)), int(rng.choice([16, 64, 144, 400])), int(rng.integers(3, 30))) for i in range(13)]


def _dp_run_shard(page_ids):
    """One rank: its pages through the continuous batcher over a stand-in slot engine -> padded ids + lengths."""
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    sys.path.insert(0, str(ROOT / "tests"))
    from fakes import FakeSlotEngine
    job = _dp_job_pages()
    eng = FakeSlotEngine(lambda prompt: int(prompt[0]) * 1000 + np.arange(64), max_batch=3, max_patches=500, max_prefill_tokens=96, max_seq_len=256)
    reqs = []
    for p in page_ids:
        first, n_tok, patches, cap = job[p]
        reqs.append(Request(np.full(n_tok, first, np.int32), np.zeros((patches, 4), np.float32), np.array([[1, patches // 4, 4]]), cap))
    outs = ContinuousBatcher(eng, chunk=5).run(reqs)
    ids = np.zeros((len(outs), 64), np.int32)
    lens = np.zeros((len(outs),), np.int32)
    for j, o in enumerate(outs):
        ids[j, :len(o)], lens[j] = o, len(o)
    return ids, lens


def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dots_ocr_amd import dp as _dp
    from test_host_cpu import _dp_job_pages, _dp_run_shard
    costs = [_dp.page_cost(patches, cap) for (_, _, patches, cap) in _dp_job_pages()]
    mine = _dp.shard_pages(costs, world)[rank]
    ids, lens = _dp_run_shard(mine)
    q.put((rank, _dp.gather_token_ids(ids, lens, page_index=mine)))
    dist.destroy_process_group()


def test_data_parallel_job_equals_single_rank_world_size_2_gloo():
    """Pages sharded by cost over 2 ranks, each shard continuously batched, results gathered: every rank ends up with the
    whole job in page order and it equals the single-rank run (result equality vs 1 GPU, any page order)."""
    import torch.multiprocessing as mp
    single_ids, single_lens = _dp_run_shard(list(range(len(_dp_job_pages()))))
    want = [(p, single_ids[p, :single_lens[p]].tolist()) for p in range(len(single_lens))]
    assert all(len(t) == min(cap, 64) and t[0] == first * 1000 for (_, t), (first, _, _, cap) in zip(want, _dp_job_pages()))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0] == want and got[1] == want


# ---- round 6: the mixed64 job of bench.py at world_size 8 (gloo, stand-in slot engine), static LPT shard and shared page queue
def _mixed64_job():
    """bench.py's configs[3] page mix (seed 2025): (first prompt token, prompt tokens, patches, cap, cost) per page.  Caps vary (seeded) so that the
    ranks' shards do not finish together — the case the shared queue exists for."""
    sys.path.insert(0, str(ROOT))
    import bench
    from dots_ocr_amd import dp as _dp
    from dots_ocr_amd.image_utils import smart_resize
    cfg = DotsConfig()
    rng = np.random.default_rng(64)
    job = []
    for i, (w, h) in enumerate(bench.mixed_pages(64)):
        rh, rw = smart_resize(h, w, 28, cfg.min_pixels, cfg.max_pixels)
        n = (rh // 14) * (rw // 14)
        cap = int(rng.integers(8, 48))
        job.append((100 + i, 12 + i % 7, n, cap, _dp.page_cost(n, 1024)))
    return job


def _mixed64_requests(page_ids):
    from dots_ocr_amd.scheduler import Request
    job = _mixed64_job()
    return [Request(np.full(job[p][1], job[p][0], np.int32), np.zeros((job[p][2], 1), np.float32), np.array([[1, job[p][2] // 4, 4]]), job[p][3]) for p in page_ids]


def _mixed64_engine():
    sys.path.insert(0, str(ROOT / "tests"))
    from fakes import FakeSlotEngine
    return FakeSlotEngine(lambda prompt: int(prompt[0]) * 1000 + np.arange(64), max_batch=8, max_patches=8 * 35000, max_prefill_tokens=512, max_seq_len=256)


def _pad(outs):
    ids = np.zeros((len(outs), 64), np.int32)
    lens = np.zeros((len(outs),), np.int32)
    for j, o in enumerate(outs):
        ids[j, :len(o)], lens[j] = o, len(o)
    return ids, lens


def _mixed64_worker(rank, world, port, q, queue_mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dots_ocr_amd import dp as _dp
    from dots_ocr_amd.scheduler import ContinuousBatcher
    from test_host_cpu import _mixed64_engine, _mixed64_job, _mixed64_requests, _pad
    costs = [c for (_, _, _, _, c) in _mixed64_job()]
    cb = ContinuousBatcher(_mixed64_engine(), chunk=4, prefetch=2)
    if queue_mode:
        pq = _dp.PageQueue(costs, store=_dp.PageQueue.default_store(), world_size=world)
        assert pq.store is not None and pq.max_take == 4
        done = cb.run_pull(lambda k: [(p, r) for p, r in zip(*(lambda ps: (ps, _mixed64_requests(ps)))(pq.take(k)))])
        mine = sorted(done)
        ids, lens = _pad([done[p] for p in mine])
    else:
        mine = _dp.shard_pages(costs, world)[rank]
        ids, lens = _pad(cb.run(_mixed64_requests(mine)))
    q.put((rank, mine, _dp.gather_token_ids(ids, lens, page_index=mine)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("queue_mode", [False, True])
def test_mixed64_job_over_8_ranks_equals_one_rank_gloo(queue_mode):
    """bench.py's mixed64 sharding path at the world size the driver's scaling run uses.  8 gloo ranks, the configs[3] page
    mix, a stand-in slot engine per rank: (a) the static cost shard — LPT max / mean load <= 1.05 on the seed-2025 mix — and (b) the shared page
    queue (dp.PageQueue over the process group's store: every page handed out exactly once, ranks pull as their slots drain); either way every
    rank ends with the whole job in page order, equal to the single-rank run."""
    import torch.multiprocessing as mp
    from dots_ocr_amd import dp as _dp
    from dots_ocr_amd.scheduler import ContinuousBatcher
    job = _mixed64_job()
    costs = [c for (_, _, _, _, c) in job]
    shards = _dp.shard_pages(costs, 8)
    loads = [sum(costs[i] for i in sh) for sh in shards]
    assert sorted(i for sh in shards for i in sh) == list(range(64))
    assert max(loads) / (sum(loads) / 8) <= 1.05, loads
    outs = ContinuousBatcher(_mixed64_engine(), chunk=4, prefetch=2).run(_mixed64_requests(range(64)))
    want = [(p, o.tolist()) for p, o in enumerate(outs)]
    assert all(len(t) == job[p][3] and t[0] == job[p][0] * 1000 for p, t in want)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000 + (7 if queue_mode else 0)
    procs = [ctx.Process(target=_mixed64_worker, args=(r, 8, port, q, queue_mode)) for r in range(8)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(8)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    taken = sorted(i for _, mine, _ in got for i in mine)
    assert taken == list(range(64)), "every page exactly once over the ranks"
    for _, _, gathered in got:
        assert gathered == want
    # (which rank drew which page depends on the ranks' timing — here the stand-in engines are instant — and must not matter)


def test_page_queue_single_process_serves_the_cost_order_once():
    from dots_ocr_amd import dp as _dp
    pq = _dp.PageQueue([1.0, 5.0, 3.0, 5.0, 0.5])
    assert pq.take(2) == [1, 3] and pq.take(1) == [2] and pq.take(4) == [0, 4] and pq.take(3) == [] and pq.take() == []
    pq = _dp.PageQueue(list(range(64)), world_size=8)                 # one call: at most half a rank's fair share
    assert pq.max_take == 4 and pq.take(34) == [63, 62, 61, 60] and pq.take(1) == [59]


def test_markdown_post_processing_matches_reference_goldens():
    """get_formula_in_markdown / clean_text / layoutjson2md / fix_streamlit_formulas == the reference functions
    (dots_ocr/utils/format_transformer.py) on every case of tests/golden/format_transformer.json."""
    from dots_ocr_amd import format_transformer as ft
    gold = json.loads((GOLD / "format_transformer.json").read_text())
    for text, want in gold["get_formula_in_markdown"]:
        assert ft.get_formula_in_markdown(text) == want, text
    for text, want in gold["clean_text"]:
        assert ft.clean_text(text) == want, text
    for text, want in gold["fix_streamlit_formulas"]:
        assert ft.fix_streamlit_formulas(text) == want, text
    for cells, no_hf, want in gold["layoutjson2md"]:
        assert ft.layoutjson2md(None, cells, "text", no_hf) == want, cells
    # the cases the reduced round-1 stand-in got wrong
    assert ft.get_formula_in_markdown("$x^2$") == "$x^2$" and ft.get_formula_in_markdown("E = mc") == "E = mc"
    assert ft.clean_text("`$x$`") == "$x$"


def test_output_cleaner_matches_reference_goldens():
    """OutputCleaner().clean_model_output == the reference class (dots_ocr/utils/output_cleaner.py) on valid, truncated,
    glued, repeated and degenerate layout JSON (tests/golden/output_cleaner.json, 151 inputs incl. a seeded mutation sweep)."""
    from dots_ocr_amd.output_cleaner import OutputCleaner
    gold = json.loads((GOLD / "output_cleaner.json").read_text())
    assert len(gold) > 100
    for inp, want in gold:
        assert OutputCleaner().clean_model_output(inp) == want, inp if not isinstance(inp, str) else inp[:200]


def test_post_process_output_salvages_truncated_generation():
    """A page cut off at max_new_tokens: the reference writes the recovered cells' text, not the broken JSON
    (layout_utils.py:221-228)."""
    from PIL import Image
    from dots_ocr_amd.layout_utils import post_process_output
    img = Image.new("RGB", (280, 280), "white")
    broken = '[{"bbox": [1, 2, 30, 40], "category": "Text", "text": "first"}, {"bbox": [5, 50, 60, 70], "category": "Text", "text": "second"}, {"bbox": [5, 80, 60'
    out, filtered = post_process_output(broken, "prompt_layout_all_en", img, img)
    assert filtered and out == "first\n\nsecond"
    cells, filtered = post_process_output('[{"bbox": [1, 2, 30, 40], "category": "Text", "text": "ok"}]', "prompt_layout_all_en", img, img)
    assert not filtered and cells[0]["text"] == "ok"


def test_demo_display_helpers_resize_like_the_reference(tmp_path):
    """dots_ocr.utils.demo_utils.display.read_image (imported by the reference's demo UIs; reference display.py:27-62): longer side
    -> 1024 (or kept with use_native), the other side truncated, original size returned; sizes checked against values computed by
    the reference function in this container."""
    from PIL import Image
    from dots_ocr.utils.demo_utils.display import is_valid_image_path, read_image
    want = {(300, 200): (1024, 682), (200, 300): (682, 1024), (256, 256): (1024, 1024), (1999, 777): (1024, 398)}
    for (w, h), size in want.items():
        p = tmp_path / f"im_{w}x{h}.png"
        Image.new("RGB", (w, h), (1, 2, 3)).save(p)
        img, ow, oh = read_image(str(p))
        assert img.size == size and (ow, oh) == (w, h)
        img, ow, oh = read_image(str(p), use_native=True)
        assert max(img.size) == max(w, h) and (ow, oh) == (w, h)
    (tmp_path / "notes.txt").write_text("x")
    assert not is_valid_image_path(str(tmp_path / "notes.txt")) and not is_valid_image_path(str(tmp_path / "missing.png"))
    with pytest.raises(FileNotFoundError):
        read_image(str(tmp_path / "missing.png"))


def test_draw_layout_on_image_follows_the_reference_semantics():
    """reference layout_utils.py:30-110: category colours, 30 % translucent fill or outline, "<order>_<category>" labels, boxes given
    in resized coordinates scaled back, draw_bbox=False leaves the page pixels alone except for the labels."""
    from dots_ocr.utils.layout_utils import dict_layout_type_to_color, draw_layout_on_image
    page = Image.new("RGB", (400, 300), (255, 255, 255))
    cells = [{"bbox": [10, 10, 200, 100], "category": "Title", "text": "x"}, {"bbox": [20, 120, 380, 280], "category": "Table"}]
    out = draw_layout_on_image(page, cells)
    assert out.size == page.size and out.mode == "RGB" and page.getpixel((50, 50)) == (255, 255, 255)          # input untouched
    r, g, b = dict_layout_type_to_color["Title"][:3]
    blend = tuple(round(255 * 0.7 + c * 0.3) for c in (r, g, b))
    assert all(abs(a - e) <= 2 for a, e in zip(out.getpixel((50, 50)), blend))                                   # 30 % fill
    assert out.getpixel((5, 5)) == (255, 255, 255) and out.getpixel((100, 200)) != (255, 255, 255)
    edge = draw_layout_on_image(page, cells, fill_bbox=False)
    assert edge.getpixel((10, 50)) == (r, g, b) and edge.getpixel((50, 50)) == (255, 255, 255)                 # outline only
    scaled = draw_layout_on_image(page, cells, resized_height=600, resized_width=800, fill_bbox=False)
    assert scaled.getpixel((5, 25)) == (r, g, b)                                                                 # x0 = 10 / 2
    labels_only = draw_layout_on_image(page, cells, draw_bbox=False)
    assert labels_only.getpixel((50, 50)) == (255, 255, 255)
    unknown = draw_layout_on_image(page, [{"bbox": [0, 0, 50, 50], "category": "Sidebar"}])                      # unlisted category: green
    assert unknown.getpixel((25, 25))[1] > unknown.getpixel((25, 25))[0]


# ---------------------------------------------------------------------------------------------- PDF rasterisation
def _pdf(objects, compressed=()):
    """Serialise {num: (dict_source, stream_bytes | None)} into a PDF; the numbers in `compressed` go into one object stream (PDF 1.5)."""
    import zlib
    out = bytearray(b"%PDF-1.5\n%\xe2\xe3\xcf\xd3\n")
    for num, (src, stream) in objects.items():
        if num in compressed:
            continue
        out += b"%d 0 obj\n%s\n" % (num, src)
        if stream is not None:
            out += b"stream\n" + stream + b"\nendstream\n"
        out += b"endobj\n"
    if compressed:
        bodies, head, off = [], [], 0
        for num in compressed:
            body = objects[num][0] + b"\n"
            head.append(b"%d %d" % (num, off))
            bodies.append(body)
            off += len(body)
        h = b" ".join(head) + b"\n"
        raw = zlib.compress(h + b"".join(bodies))
        out += b"90 0 obj\n<< /Type /ObjStm /N %d /First %d /Length %d /Filter /FlateDecode >>\nstream\n" % (len(compressed), len(h), len(raw)) + raw + b"\nendstream\nendobj\n"
    out += b"trailer\n<< /Root 1 0 R >>\n%%EOF\n"
    return bytes(out)


def test_pdf_rasteriser_scanned_pages_like_the_reference(tmp_path):
    """reference dots_ocr/utils/doc_utils.py:20-60 (PyMuPDF): 200 dpi render, > 4500 px falls back to 72 dpi, page range selection.
    PyMuPDF is absent here, so the built-in reader renders image-only (scanned) PDFs: a 3-page JPEG PDF written by Pillow, a
    hand-built PDF 1.5 (object stream, Flate + PNG-predictor RGB image placed with a cm matrix on a larger page, invisible OCR text
    layer), the oversize fallback, and the refusal of pages it cannot render faithfully."""
    import zlib
    from PIL import Image, ImageDraw
    from dots_ocr_amd import doc_utils as du
    from dots_ocr.utils.doc_utils import load_images_from_pdf as ref_name_load            # the drop-in import path
    assert ref_name_load is du.load_images_from_pdf

    def page(i, size=(1654, 2339)):
        im = Image.new("RGB", size, (255, 255, 255))
        d = ImageDraw.Draw(im)
        for y in range(60, size[1] - 60, 90):
            d.text((80, y), f"page {i} line {y}: the quick brown fox", fill=(0, 0, 0))
        d.rectangle([100, 100, 300 + 80 * i, 220], outline=(200, 0, 0), width=6)
        return im
    pages = [page(i) for i in range(3)]
    f = tmp_path / "scan.pdf"
    pages[0].save(f, "PDF", resolution=200.0, save_all=True, append_images=pages[1:])
    got = du.load_images_from_pdf(str(f))
    assert [g.size for g in got] == [(1654, 2339)] * 3 and all(g.mode == "RGB" for g in got)
    for a, b in zip(pages, got):                              # JPEG inside: close, not equal
        assert np.abs(np.asarray(a, np.int16) - np.asarray(b, np.int16)).mean() < 1.0
    assert [g.size for g in du.load_images_from_pdf(str(f), start_page_id=1, end_page_id=9)] == [(1654, 2339)] * 2
    assert len(du.load_images_from_pdf(str(f), start_page_id=2)) == 1 and len(du.load_images_from_pdf(str(f), end_page_id=0)) == 1
    assert du.load_images_from_pdf(str(f), dpi=72)[0].size == (596, 843)                  # ceil(595.44), ceil(842.04)

    # hand-built: 300 x 200 RGB gradient, Flate + PNG "Up" predictor, drawn at (50, 80) size 300 x 200 pt on a 400 x 400 pt page
    w, h = 300, 200
    img = np.zeros((h, w, 3), np.uint8)
    img[..., 0] = np.arange(w)[None, :] % 256
    img[..., 1] = (np.arange(h)[:, None] * 255 // (h - 1)).astype(np.uint8)
    img[..., 2] = 77
    rows, prev = bytearray(), np.zeros((w * 3,), np.uint8)
    for r in range(h):
        cur = img[r].reshape(-1)
        rows += bytes([2]) + ((cur.astype(np.int16) - prev.astype(np.int16)) & 255).astype(np.uint8).tobytes()
        prev = cur
    raw = zlib.compress(bytes(rows))
    content = b"q 300 0 0 200 50 80 cm /Im0 Do Q BT 3 Tr /F1 12 Tf (hidden ocr layer) Tj ET"
    objs = {
        1: (b"<< /Type /Catalog /Pages 2 0 R >>", None),
        2: (b"<< /Type /Pages /Kids [3 0 R] /Count 1 /MediaBox [0 0 400 400] >>", None),
        3: (b"<< /Type /Page /Parent 2 0 R /Resources << /XObject << /Im0 4 0 R >> >> /Contents 5 0 R >>", None),
        4: (b"<< /Type /XObject /Subtype /Image /Width 300 /Height 200 /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode "
            b"/DecodeParms << /Predictor 15 /Colors 3 /BitsPerComponent 8 /Columns 300 >> /Length %d >>" % len(raw), raw),
        5: (b"<< /Length %d >>" % len(content), content),
    }
    data = _pdf(objs, compressed=(1, 2, 3))
    doc = du.PdfDocument(data)
    assert doc.page_count == 1
    out = np.asarray(du.fitz_doc_to_image(doc[0], target_dpi=72))                          # 1 pt = 1 px: no resampling
    assert out.shape == (400, 400, 3)
    assert np.array_equal(out[400 - 80 - 200:400 - 80, 50:350], img)                       # PDF y axis points up
    assert (out[:120] == 255).all() and (out[:, :50] == 255).all() and (out[:, 350:] == 255).all() and (out[320:] == 255).all()
    big = np.asarray(du.fitz_doc_to_image(doc[0], target_dpi=200))
    assert big.shape == (1112, 1112, 3) and tuple(big[1111 - 300, 300]) != (255, 255, 255) and tuple(big[5, 5]) == (255, 255, 255)

    # > 4500 px at the target dpi -> 72 dpi (reference doc_utils.py:33-36)
    objs[2] = (b"<< /Type /Pages /Kids [3 0 R] /Count 1 /MediaBox [0 0 2000 1700] >>", None)
    assert du.fitz_doc_to_image(du.PdfDocument(_pdf(objs))[0], target_dpi=200).size == (2000, 1700)

    # visible text / vector painting: refused, not rendered wrongly
    for bad in (b"BT /F1 12 Tf (visible) Tj ET", b"0 0 100 100 re f"):
        objs[5] = (b"<< /Length %d >>" % len(bad), bad)
        with pytest.raises(du.PdfContentNotSupported):
            du.fitz_doc_to_image(du.PdfDocument(_pdf(objs))[0])


def test_continuous_batcher_look_ahead_prefetches_the_next_towers_with_a_fake_engine():
    """Scheduler logic only: with prefetch = k the towers of the next k queued image requests are started on the side stream while the slots
    decode, that group is admitted as a whole (take + prefill, no tower call) as soon as it has k free slots, nothing overtakes it, text-only
    requests go through the ordinary admission, and every request still gets exactly its own tokens."""
    import numpy as np
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    from fakes import FakeSlotEngine

    def req(first, n_tok, cap, patches=0):
        ids = np.full(n_tok, first, np.int32)
        if patches:
            return Request(ids, np.zeros((patches, 4), np.float32), np.array([[1, patches // 2, 2]]), cap)
        return Request(ids, None, None, cap)

    def want(reqs):
        return [list(range(r.input_ids[0], r.input_ids[0] + r.max_new_tokens)) for r in reqs]
    for k in (1, 2, 3):
        eng = FakeSlotEngine(lambda prompt: int(prompt[0]) + np.arange(200), max_batch=3, max_patches=100, max_prefill_tokens=64, max_seq_len=256)
        cb = ContinuousBatcher(eng, eos_ids=(), chunk=4, prefetch=k)
        reqs = [req(10, 8, 9, 20), req(20, 8, 5, 20), req(30, 8, 13, 20), req(40, 8, 6, 30), req(50, 8, 3), req(60, 8, 7, 20), req(70, 8, 4, 40), req(80, 8, 9, 10)]
        out = cb.run(reqs)
        assert [o.tolist() for o in out] == want(reqs), k
        assert cb.idle and not eng.slots and not getattr(eng, "_pref", None)
        kinds = [e[0] for e in eng.log]
        assert kinds.count("prefetch") == kinds.count("take") >= 2
        # every take is followed at once by the prefill of exactly the prefetched group
        for i, e in enumerate(eng.log):
            if e[0] == "take":
                assert eng.log[i + 1][0] == "prefill"
        # the first admission is the ordinary one (the engine is empty: its tower cannot be hidden behind anything)
        assert kinds[0] == "vit" and kinds[1] == "prefill"
        # towers run ahead of their admission: a prefetch is logged while slots are occupied, and decode chunks happen between prefetch and take
        i0 = kinds.index("prefetch")
        assert "decode" in kinds[i0:kinds.index("take", i0)]
        # patches seen by prefetch + vit calls == all image patches, each exactly once
        assert sum(e[1] for e in eng.log if e[0] in ("vit", "prefetch")) == sum(r.n_patches() for r in reqs)
    # prefetch = 0 is today's behaviour: no prefetch calls at all
    eng = FakeSlotEngine(lambda prompt: int(prompt[0]) + np.arange(200), max_batch=3, max_patches=100, max_prefill_tokens=64, max_seq_len=256)
    ContinuousBatcher(eng, eos_ids=(), chunk=4).run([req(10, 8, 9, 20), req(20, 8, 5, 20)])
    assert not any(e[0] in ("prefetch", "take") for e in eng.log)


def test_pdf_reader_resource_limits_on_untrusted_files(monkeypatch):
    """the built-in PDF reader bounds what a hostile file can make it allocate or recurse into: a Flate bomb, a /Kids cycle,
    an object stream with a lying header and an image placed far larger than the page all fail with ValueError."""
    import zlib
    from dots_ocr_amd import doc_utils as du

    def build(objs):
        out, offs = bytearray(b"%PDF-1.5\n"), {}
        for num, (dic, stream) in objs.items():
            offs[num] = len(out)
            out += b"%d 0 obj\n" % num + dic
            if stream is not None:
                out += b"\nstream\n" + stream + b"\nendstream"
            out += b"\nendobj\n"
        out += b"trailer\n<< /Root 1 0 R /Size %d >>\n%%%%EOF\n" % (max(objs) + 1)
        return bytes(out)

    # 1. decompression bomb: 64 MiB of zeros in ~64 KiB, cap lowered to 1 MiB for the test
    monkeypatch.setattr(du, "MAX_STREAM_BYTES", 1 << 20)
    bomb = zlib.compress(b"\0" * (64 << 20), 9)
    content = b"q 100 0 0 100 0 0 cm /Im0 Do Q"
    objs = {1: (b"<< /Type /Catalog /Pages 2 0 R >>", None),
            2: (b"<< /Type /Pages /Kids [3 0 R] /Count 1 /MediaBox [0 0 100 100] >>", None),
            3: (b"<< /Type /Page /Parent 2 0 R /Resources << /XObject << /Im0 4 0 R >> >> /Contents 5 0 R >>", None),
            4: (b"<< /Type /XObject /Subtype /Image /Width 8192 /Height 8192 /ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /FlateDecode "
                b"/Length %d >>" % len(bomb), bomb),
            5: (b"<< /Length %d >>" % len(content), content)}
    with pytest.raises(ValueError, match="inflates beyond"):
        du.PdfDocument(build(objs))[0].render(72)
    # 2. a page tree that contains itself
    cyc = {1: (b"<< /Type /Catalog /Pages 2 0 R >>", None),
           2: (b"<< /Type /Pages /Kids [3 0 R] /Count 1 /MediaBox [0 0 100 100] >>", None),
           3: (b"<< /Type /Pages /Kids [2 0 R] /Count 1 >>", None)}
    with pytest.raises(ValueError, match="page tree"):
        du.PdfDocument(build(cyc))
    # 3. object stream whose header claims more objects than it has bytes for
    body = zlib.compress(b"7 0 << /Type /Catalog >>")
    bad = {1: (b"<< /Type /Catalog /Pages 2 0 R >>", None),
           2: (b"<< /Type /Pages /Kids [] /Count 0 >>", None),
           6: (b"<< /Type /ObjStm /N 100000000 /First 4 /Filter /FlateDecode /Length %d >>" % len(body), body)}
    with pytest.raises(ValueError, match="object stream"):
        du.PdfDocument(build(bad))
    # 4. an image placed 100x larger than its page
    monkeypatch.setattr(du, "MAX_STREAM_BYTES", 512 << 20)
    px = zlib.compress(bytes(16 * 16))
    big = b"q 10000 0 0 10000 0 0 cm /Im0 Do Q"
    huge = {1: (b"<< /Type /Catalog /Pages 2 0 R >>", None),
            2: (b"<< /Type /Pages /Kids [3 0 R] /Count 1 /MediaBox [0 0 100 100] >>", None),
            3: (b"<< /Type /Page /Parent 2 0 R /Resources << /XObject << /Im0 4 0 R >> >> /Contents 5 0 R >>", None),
            4: (b"<< /Type /XObject /Subtype /Image /Width 16 /Height 16 /ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /FlateDecode "
                b"/Length %d >>" % len(px), px),
            5: (b"<< /Length %d >>" % len(big), big)}
    with pytest.raises(ValueError, match="exceeds the page raster"):
        du.PdfDocument(build(huge))[0].render(72)


def test_pdf_rasteriser_colour_modes_rotation_and_several_images_per_page():
    """What scanners really produce: gray / RGB / CMYK JPEG, bilevel Group-4 fax (CCITTFaxDecode), palette images; a /Rotate 90 page;
    a page assembled from two image strips."""
    import io
    import zlib
    from PIL import Image, ImageDraw
    from dots_ocr_amd import doc_utils as du
    base = Image.new("RGB", (400, 300), (255, 255, 255))
    d = ImageDraw.Draw(base)
    d.rectangle([50, 40, 300, 200], fill=(200, 30, 30))
    d.text((60, 220), "hello scanned world", fill=(0, 0, 0))
    for mode, tol in (("L", 0.5), ("1", 0.0), ("P", 0.0), ("CMYK", 0.5), ("RGB", 1.5)):
        im = base.convert(mode)
        buf = io.BytesIO()
        im.save(buf, "PDF", resolution=72.0)
        out = du.fitz_doc_to_image(du.PdfDocument(buf.getvalue())[0], target_dpi=72)
        assert out.size == (400, 300) and out.mode == "RGB"
        assert np.abs(np.asarray(out, np.int16) - np.asarray(im.convert("RGB"), np.int16)).mean() <= tol, mode

    def raw_image(arr):                                   # uncompressed-then-deflated 8-bit RGB image XObject
        raw = zlib.compress(arr.tobytes())
        return (b"<< /Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode /Length %d >>"
                % (arr.shape[1], arr.shape[0], len(raw)), raw)
    top = np.zeros((100, 200, 3), np.uint8); top[..., 0] = 250
    bot = np.zeros((50, 200, 3), np.uint8); bot[..., 2] = 250
    content = b"q 200 0 0 100 0 50 cm /T Do Q q 200 0 0 50 0 0 cm /B Do Q"
    objs = {
        1: (b"<< /Type /Catalog /Pages 2 0 R >>", None),
        2: (b"<< /Type /Pages /Kids [3 0 R] /Count 1 >>", None),
        3: (b"<< /Type /Page /Parent 2 0 R /MediaBox [0 0 200 150] /Rotate 90 /Resources << /XObject << /T 4 0 R /B 6 0 R >> >> /Contents 5 0 R >>", None),
        4: raw_image(top), 5: (b"<< /Length %d >>" % len(content), content), 6: raw_image(bot),
    }
    page = np.asarray(du.fitz_doc_to_image(du.PdfDocument(_pdf(objs))[0], target_dpi=72))
    assert page.shape == (200, 150, 3)                    # rotated clockwise by 90 degrees
    upright = np.rot90(page, 1)                           # undo: counter-clockwise
    assert (upright[:100, :, 0] == 250).all() and (upright[:100, :, 2] == 0).all()        # red strip on top
    assert (upright[100:, :, 2] == 250).all() and (upright[100:, :, 0] == 0).all()        # blue strip below


def test_scheduler_surfaces_kv_truncation_and_full_reservation_never_truncates():
    """with on-demand paging a dry pool ends a sequence at what its pages hold (P positions -> P + 1 tokens); the batcher
    marks such requests `kv_truncated` (the server answers finish_reason "kv_pool_exhausted") and counts them; `headroom_pages=None`
    is the full-reservation policy of rounds 1-2: fewer sequences in flight, nothing truncated."""
    from fakes import FakePagedEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    script = lambda prompt: int(prompt[0]) * 1000 + np.arange(400)
    mk = lambda: [Request(np.full(40, i, np.int32), None, None, 300) for i in range(1, 5)]          # 4 x (40 + 300) tokens = 4 x 6 pages by worst case
    eng = FakePagedEngine(script, pool_pages=12, max_batch=4, max_patches=100, max_prefill_tokens=1 << 20, max_seq_len=1024)
    cb = ContinuousBatcher(eng, chunk=8, headroom_pages=0)
    reqs = mk()
    outs = cb.run(reqs)
    assert cb.kv_truncated >= 1 and eng.capped >= 1
    for r, o in zip(reqs, outs):
        pages_tokens = len(o) + 40 - 1                              # KV positions its tokens needed
        if r.kv_truncated:
            assert len(o) < 300 and pages_tokens % 64 == 0, (len(o),)           # ended exactly at what whole pages hold
        else:
            assert len(o) == 300
        assert o.tolist() == (int(r.input_ids[0]) * 1000 + np.arange(len(o))).tolist()
    assert eng.kv_pool_info() == (12, 12)
    eng2 = FakePagedEngine(script, pool_pages=12, max_batch=4, max_patches=100, max_prefill_tokens=1 << 20, max_seq_len=1024)
    cb2 = ContinuousBatcher(eng2, chunk=8, headroom_pages=None)
    reqs2 = mk()
    outs2 = cb2.run(reqs2)
    assert cb2.kv_truncated == 0 and eng2.capped == 0 and all(len(o) == 300 for o in outs2) and not any(r.kv_truncated for r in reqs2)
    assert max(len(x[2]) for x in eng2.log if x[0] == "decode") == 2              # 12 pages / 6 per sequence: two at a time


def test_scheduler_keeps_failed_groups_findable_for_the_callers_error_handling():
    """a request popped from `pending` must not vanish when the engine call that was to admit it raises — the server fails
    the futures it finds in running / pending / _ahead, anything else hangs its HTTP request for ever."""
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request

    class Failing(FakeSlotEngine):
        fail_prefetch = fail_take = False
        def vit_prefetch(self, *a, **k):
            if self.fail_prefetch:
                raise RuntimeError("tower launch failed")
            return super().vit_prefetch(*a, **k)
        def vit_take(self):
            if self.fail_take:
                raise RuntimeError("no rows")
            return super().vit_take()
    mk = lambda i: Request(np.full(8, i, np.int32), np.zeros((16, 4), np.float32), np.asarray([[1, 4, 4]]), 20, tag=i)
    eng = Failing(lambda prompt: int(prompt[0]) + np.arange(64), max_batch=2, max_patches=100, max_prefill_tokens=64, max_seq_len=256)
    cb = ContinuousBatcher(eng, chunk=4, prefetch=2, tower_steps_per_page=1)      # a tower as short as a decode step: the look-ahead horizon is two chunks
    for i in range(1, 5):
        cb.submit(mk(i))
    eng.fail_prefetch = True
    with pytest.raises(RuntimeError, match="tower launch failed"):
        cb.step()                       # admits 1, 2 — then the look-ahead (3: both slots are busy and far from their caps) fails
    assert sorted(r.tag for _, r in cb.pending) == [3, 4] and not cb._ahead
    eng.fail_prefetch = False
    cb.step()                            # look-ahead succeeds now: ONE request, the engine is full (no group larger than the free slots)
    assert [r.tag for _, r in cb._ahead] == [3]
    eng.fail_take = True
    with pytest.raises(RuntimeError, match="no rows"):
        for _ in range(50):              # drain 1, 2; the admission of the prefetched group then fails at vit_take
            cb.step()
    assert not cb._ahead and sorted(r.tag for _, r in cb.pending) == [3, 4]
    # a request that can never be admitted stays at the head of the queue when step() raises
    eng3 = FakeSlotEngine(lambda prompt: np.arange(8), max_batch=1, max_patches=100, max_prefill_tokens=64, max_seq_len=256)
    cb3 = ContinuousBatcher(eng3)
    cb3.pending.append((7, Request(np.zeros(80, np.int32), None, None, 4, tag="too long for max_prefill_tokens")))
    cb3.plan_admission = lambda: []
    with pytest.raises(RuntimeError, match="cannot be admitted"):
        cb3.step()
    assert len(cb3.pending) == 1


def test_scheduler_requeues_the_group_when_the_ordinary_admission_fails():
    """plan_admission() pops the group from `pending`; if vit_forward or slots_prefill then raises, the requests
    must go back to the head of the queue (in order) — the server's failure handling walks pending / running / _ahead only, so a
    request held by none of them would hang its HTTP call.  Covers the first group after start-up, text-only requests, look_ahead=0."""
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request

    class Failing(FakeSlotEngine):
        fail_vit = fail_prefill = False
        def vit_forward(self, *a, **k):
            if self.fail_vit:
                raise RuntimeError("tower failed")
            return super().vit_forward(*a, **k)
        def slots_prefill(self, *a, **k):
            if self.fail_prefill:
                raise RuntimeError("prefill failed")
            return super().slots_prefill(*a, **k)
    img = lambda i: Request(np.full(8, i, np.int32), np.zeros((16, 4), np.float32), np.asarray([[1, 4, 4]]), 6, tag=i)
    txt = lambda i: Request(np.full(8, i, np.int32), None, None, 6, tag=i)
    for fail, make in (("fail_vit", img), ("fail_prefill", img), ("fail_prefill", txt)):
        eng = Failing(lambda prompt: int(prompt[0]) + np.arange(64), max_batch=2, max_patches=100, max_prefill_tokens=64, max_seq_len=256)
        cb = ContinuousBatcher(eng, chunk=4, prefetch=0)
        ids = [cb.submit(make(i)) for i in range(1, 4)]
        setattr(eng, fail, True)
        with pytest.raises(RuntimeError, match="failed"):
            cb.step()
        assert [rid for rid, _ in cb.pending] == ids and not cb.running and not cb._ahead and not eng.slots      # nothing lost, order kept
        setattr(eng, fail, False)
        out = {}
        while not cb.idle:
            for rid, r, toks in cb.step():
                out[rid] = (r.tag, toks.tolist())
        assert sorted(out) == ids and all(out[i][1] == (out[i][0] + np.arange(6)).tolist() for i in ids)


def test_scheduler_full_reservation_holds_on_the_look_ahead_paths_too():
    """with headroom_pages=None nothing may ever be truncated by a dry pool — also when image requests enter through
    the look-ahead (prefetch > 0, the server default); a lone request whose worst case exceeds the pool is refused at submit()."""
    from fakes import FakePagedEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    script = lambda prompt: int(prompt[0]) * 1000 + np.arange(400)
    mk = lambda i, cap=300: Request(np.full(40, i, np.int32), np.zeros((16, 4), np.float32), np.asarray([[1, 4, 4]]), cap)
    eng = FakePagedEngine(script, pool_pages=12, max_batch=4, max_patches=100, max_prefill_tokens=1 << 20, max_seq_len=1024)
    cb = ContinuousBatcher(eng, chunk=8, headroom_pages=None, prefetch=4)
    reqs = [mk(i) for i in range(1, 7)]                    # 6 x (40 + 300) tokens = 6 pages each by worst case: two at a time in 12 pages
    outs = cb.run(reqs)
    assert cb.kv_truncated == 0 and eng.capped == 0 and all(len(o) == 300 for o in outs)
    assert max(len(x[2]) for x in eng.log if x[0] == "decode") == 2
    assert any(x[0] == "prefetch" for x in eng.log)         # the look-ahead path was exercised
    with pytest.raises(ValueError, match="full\\s+reservation|under full"):
        cb.submit(mk(9, cap=900))                          # 40 + 900 tokens = 15 pages > 12


def test_scheduler_look_ahead_group_is_capped_by_the_slots_that_are_or_will_soon_be_free():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    mk = lambda i, cap: Request(np.full(8, i, np.int32), np.zeros((16, 4), np.float32), np.asarray([[1, 4, 4]]), cap, tag=i)
    eng = FakeSlotEngine(lambda prompt: int(prompt[0]) + np.arange(4096), max_batch=4, max_patches=100, max_prefill_tokens=64, max_seq_len=8192)
    cb = ContinuousBatcher(eng, chunk=4, prefetch=4)
    for i, cap in enumerate([2000, 2000, 2000, 12, 50, 50, 50, 50], 1):
        cb.submit(mk(i, cap))
    cb.step()                                              # 1-4 admitted; every slot busy: the look-ahead takes ONE request
    assert len(cb.running) == 4 and [r.tag for _, r in cb._ahead] == [5]
    while 4 in [r.tag for _, r in cb.running.values()]:
        cb.step()
    # request 4 (12 tokens) finished: its slot went to the prefetched request at once instead of waiting for three more slots
    steps = 0
    while 5 not in [r.tag for _, r in cb.running.values()]:
        cb.step(); steps += 1
        assert steps < 3
    assert sum(1 for _, r in cb.running.values() if r.tag in (1, 2, 3)) == 3
    # equal caps (the pages of one document, EOS off): everything finishes together, so the WHOLE next group is prefetched while the
    # current one decodes — k towers last k * tower_steps_per_page steps, and all k slots are free by then
    eng2 = FakeSlotEngine(lambda prompt: int(prompt[0]) + np.arange(4096), max_batch=4, max_patches=100, max_prefill_tokens=64, max_seq_len=8192)
    cb2 = ContinuousBatcher(eng2, chunk=4, prefetch=4, tower_steps_per_page=48)
    for i in range(1, 9):
        cb2.submit(mk(i, 150))
    cb2.step()                                             # 1-4 admitted at length 0: 8 + 4 * 48 = 200 >= 150 steps to go -> all four towers ahead
    assert len(cb2.running) == 4 and [r.tag for _, r in cb2._ahead] == [5, 6, 7, 8]
    outs = []
    while not cb2.idle:
        outs += cb2.step()
    assert sorted(r.tag for _, r, _ in outs) == list(range(1, 9)) and all(len(t) == 150 for _, _, t in outs)


def test_scheduler_reused_slot_does_not_inherit_the_previous_occupants_length():
    """`_last_lens` kept a finished sequence's final length, so a request admitted into that slot looked "about to finish" to the
    look-ahead that runs right after the admission: the prefetched group was sized for slots that stayed busy and, being all-or-nothing
    (nothing may overtake it), held freed slots idle.  Wave 1 (four requests that run to 1000 tokens) leaves stale lengths of 1000 behind;
    wave 2 has caps 250 / 250 / 250 / 1000; with the stale lengths wave 3 was prefetched as ONE group of four and waited for the 1000-token
    sequence while three slots idled for 750 steps."""
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    mk = lambda i, cap: Request(np.full(8, i, np.int32), np.zeros((16, 4), np.float32), np.asarray([[1, 4, 4]]), cap, tag=i)
    eng = FakeSlotEngine(lambda prompt: int(prompt[0]) + np.arange(4096), max_batch=4, max_patches=100, max_prefill_tokens=64, max_seq_len=8192)
    cb = ContinuousBatcher(eng, chunk=4, prefetch=4, tower_steps_per_page=1)
    for i, cap in enumerate([1000] * 4 + [250, 250, 250, 1000] + [250] * 4, 1):
        cb.submit(mk(i, cap))
    outs, idle_while_waiting = [], 0
    while not cb.idle:
        outs += cb.step()
        for s, (_, r) in cb.running.items():                   # a tracked length never exceeds what its CURRENT occupant may generate
            assert cb._last_lens.get(s, 0) <= r.max_new_tokens
        if cb.pending or cb._ahead:
            idle_while_waiting += (4 - len(cb.running)) * cb.chunk
    assert sorted(r.tag for _, r, _ in outs) == list(range(1, 13)) and all(len(t) == r.max_new_tokens for _, r, t in outs)
    # wave 1 ends at 1000, wave 2's long request at 2000; wave 3 fits behind the three short ones (250 + 250 < 1000): ~2000 steps (2250 with the stale lengths)
    assert cb.decode_steps <= 2000 + 16 * cb.chunk, cb.decode_steps
    assert idle_while_waiting <= 16 * cb.chunk, idle_while_waiting


def test_scheduler_cold_start_ramp_and_tower_readiness_gate():
    """Round 5: admit_group = the look-ahead group size also for the ordinary (cold-start) admission, and a prefetched group is taken only
    when its tower has FINISHED while sequences are decoding (Engine.vit_ready): the decode loop starts after one small tower, the later
    groups' towers run beside it, no decode chunk ever queues behind a tower — and a closed set of equal caps finishes staggered."""
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request

    class Timed(FakeSlotEngine):
        tower_chunks = 3                                   # decode chunks a prefetched tower lasts
        def vit_prefetch(self, *a, **k):
            self._age = 0
            return super().vit_prefetch(*a, **k)
        def slots_decode(self, n):
            self._age = getattr(self, "_age", 0) + 1
            return super().slots_decode(n)
        def vit_ready(self):
            return self._age >= self.tower_chunks
        def vit_take(self):
            assert self._age >= self.tower_chunks or not self.slots, "a group was taken while its tower was running beside decoding sequences"
            return super().vit_take()
    mk = lambda i: Request(np.full(8, i, np.int32), np.zeros((16, 4), np.float32), np.asarray([[1, 4, 4]]), 64, tag=i)
    eng = Timed(lambda prompt: int(prompt[0]) + np.arange(4096), max_batch=8, max_patches=1000, max_prefill_tokens=640, max_seq_len=8192)
    cb = ContinuousBatcher(eng, chunk=4, prefetch=2, admit_group=2, tower_steps_per_page=8)
    for i in range(1, 13):
        cb.submit(mk(i))
    outs, occupancy = [], []
    while not cb.idle:
        outs += cb.step()
        occupancy.append(len(cb.running))
    kinds = [k for k, *_ in eng.log]
    assert kinds[:3] == ["vit", "prefill", "prefetch"] and eng.log[0][1] == 2 * 16      # the cold start admits ONE group of two pages
    # between a prefetch and its take there are >= tower_chunks decode chunks: the running sequences kept decoding beside the tower
    for i, k in enumerate(kinds):
        if k == "take":
            j = max(x for x in range(i) if kinds[x] == "prefetch")
            assert kinds[j:i].count("decode") >= Timed.tower_chunks
    assert occupancy[0] == 2 and max(occupancy) >= 6                                    # the engine fills group by group
    assert sorted(r.tag for _, r, _ in outs) == list(range(1, 13)) and all(len(t) == 64 for _, _, t in outs)


def test_first_contact_script_on_a_synthetic_checkpoint_directory(tmp_path):
    """tools/first_contact.py — the one command for the day a real checkpoint is present — run end to end on CPU
    (--no-gpu: config diff against SURVEY §8(a)'s [RECALLED] table, safetensors inventory against what the engine consumes, text side,
    and the bf16-emulated oracle decoding from the files) against a synthetic checkpoint directory: it must report the recalled values
    that differ, the tensor the engine would not consume, the tensor it would miss, an ignored key that changes the arithmetic — and exit 2."""
    import json
    import subprocess
    import sys
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.synthetic import synth_page
    from dots_ocr_amd.weights import random_state_dict, save_safetensors
    cfg = DotsConfig.tiny(layers=2, v_layers=2, vocab=1024)
    sd = random_state_dict(cfg, seed=31)
    v = cfg.vision
    base = {"hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_hidden_layers, "num_attention_heads": cfg.num_attention_heads,
            "num_key_value_heads": cfg.num_key_value_heads, "intermediate_size": cfg.intermediate_size, "vocab_size": cfg.vocab_size,
            "rope_theta": cfg.rope_theta, "rms_norm_eps": cfg.rms_norm_eps, "image_token_id": cfg.image_token_id, "attention_bias": True,
            "tie_word_embeddings": False, "pad_token_id": cfg.pad_token_id, "hidden_act": "silu", "torch_dtype": "bfloat16",
            "vision_config": {"embed_dim": v.embed_dim, "num_hidden_layers": v.num_hidden_layers, "num_attention_heads": v.num_attention_heads,
                              "intermediate_size": v.intermediate_size, "patch_size": 14, "spatial_merge_size": 2, "hidden_size": v.hidden_size}}
    root = Path(__file__).resolve().parent.parent

    def make(d, config, tensors):
        d.mkdir()
        (d / "config.json").write_text(json.dumps(config))
        (d / "generation_config.json").write_text(json.dumps({"eos_token_id": list(cfg.eos_token_ids), "do_sample": False}))
        (d / "preprocessor_config.json").write_text(json.dumps({"min_pixels": 3136, "max_pixels": 11289600}))
        save_safetensors(tensors, d / "model.safetensors")
    page = tmp_path / "page.png"
    synth_page(5, (196, 140)).save(page)

    def run(d):
        out = tmp_path / (d.name + ".json")
        p = subprocess.run([sys.executable, str(root / "tools" / "first_contact.py"), "--model-path", str(d), "--image", str(page), "--steps", "4", "--no-gpu",
                            "--prompt-mode", "prompt_ocr", "--out", str(out)], capture_output=True, text=True, timeout=600)
        return p.returncode, json.loads(out.read_text()), p.stdout + p.stderr
    # 1. a consistent checkpoint (tiny dims): nothing crashes; the only blocking item is the missing tokenizer.json
    make(tmp_path / "good", base, sd)
    rc, rep, log = run(tmp_path / "good")
    assert rc == 2 and not rep["crashed_stages"], log[-2000:]
    assert [b for b in rep["blocking"] if "tokenizer.json" in b] and len(rep["blocking"]) == 1, rep["blocking"]
    diff = {(r["where"], r["key"]) for r in rep["stages"]["1_config_diff"]["differing_recalled_values"]}
    assert ("config.json", "hidden_size") in diff and ("config.json:vision_config", "embed_dim") in diff            # tiny dims != the recalled 1536
    assert any(i["key"] == "torch_dtype" for i in rep["stages"]["1_config_diff"]["keys_the_engine_ignores"])
    inv = rep["stages"]["2_tensor_inventory"]
    assert inv["tensors_in_checkpoint"] == inv["tensors_the_engine_consumes"] == len(sd) and not inv["required_but_missing"] and not inv["present_but_unused"]
    r4 = rep["stages"]["4_run"]
    assert len(r4["oracle_tokens"]) == 4 and r4["patches"] == 140 and isinstance(r4["oracle_text"], str)
    # 2. reality differs from recollection: an activation the engine ignores, a parameter it does not model, one it needs and does not find
    bad_sd = dict(sd)
    bad_sd["vision_tower.blocks.0.attn.qkv.bias"] = torch.zeros(3 * v.embed_dim, dtype=torch.bfloat16)
    del bad_sd["model.layers.1.mlp.down_proj.weight"]
    bad_cfg = dict(base, hidden_act="gelu", rope_scaling={"type": "yarn", "factor": 4.0})
    bad_cfg["vision_config"] = dict(base["vision_config"], is_causal=True)
    make(tmp_path / "bad", bad_cfg, bad_sd)
    rc, rep, log = run(tmp_path / "bad")
    assert rc in (1, 2), log[-2000:]
    joined = " | ".join(rep["blocking"])
    for needle in ("hidden_act", "rope_scaling", "is_causal", "would NOT be consumed", "requires are absent"):
        assert needle in joined, (needle, rep["blocking"])
    assert rep["stages"]["2_tensor_inventory"]["present_but_unused"] == ["vision_tower.blocks.0.attn.qkv.bias"]
    assert rep["stages"]["2_tensor_inventory"]["required_but_missing"] == ["model.layers.1.mlp.down_proj.weight"]
