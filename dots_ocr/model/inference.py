"""OpenAI-compatible client of an external vLLM server (reference dots_ocr/model/inference.py:7-48).
Out of the accelerated path — kept so `DotsOCRParser(use_hf=False)` still works."""
import os

from dots_ocr_amd.image_utils import PILimage_to_base64


def inference_with_vllm(image, prompt, protocol="http", ip="localhost", port=8000, temperature=0.1, top_p=0.9,
                        max_completion_tokens=32768, model_name="rednote-hilab/dots.mocr", system_prompt=None, extra_body=None):
    import requests
    from openai import OpenAI        # optional dependency, imported lazily
    client = OpenAI(api_key=os.environ.get("API_KEY", "0"), base_url=f"{protocol}://{ip}:{port}/v1")
    messages = [{"role": "system", "content": system_prompt}] if system_prompt else []
    messages.append({"role": "user", "content": [
        {"type": "image_url", "image_url": {"url": PILimage_to_base64(image)}},
        {"type": "text", "text": f"<|img|><|imgpad|><|endofimg|>{prompt}"}]})
    try:
        r = client.chat.completions.create(messages=messages, model=model_name, max_completion_tokens=max_completion_tokens,
                                           temperature=temperature, top_p=top_p, **({"extra_body": extra_body} if extra_body else {}))
        return r.choices[0].message.content
    except requests.exceptions.RequestException as e:
        print(f"request error: {e}")
        return None


def inference_prompts_with_vllm(image, prompts, protocol="http", ip="localhost", port=8000, temperature=0.1, top_p=0.9,
                                max_completion_tokens=32768, model_name="rednote-hilab/dots.mocr", system_prompt=None, extra_body=None):
    """Several prompts over ONE page in one request: the dots_ocr_amd server's own `prompts` field.  The page goes through
    the vision tower and the prefill once; choice i answers prompts[i].  Returns the texts in that order, or None on a request error."""
    import requests
    from openai import OpenAI        # optional dependency, imported lazily
    client = OpenAI(api_key=os.environ.get("API_KEY", "0"), base_url=f"{protocol}://{ip}:{port}/v1")
    messages = [{"role": "system", "content": system_prompt}] if system_prompt else []
    messages.append({"role": "user", "content": [
        {"type": "image_url", "image_url": {"url": PILimage_to_base64(image)}},
        {"type": "text", "text": prompts[0]}]})
    try:
        r = client.chat.completions.create(messages=messages, model=model_name, max_completion_tokens=max_completion_tokens,
                                           temperature=temperature, top_p=top_p, extra_body={**(extra_body or {}), "prompts": list(prompts)})
        return [c.message.content for c in sorted(r.choices, key=lambda c: c.index)]
    except requests.exceptions.RequestException as e:
        print(f"request error: {e}")
        return None


def score_with_vllm(image, prompt, candidates, protocol="http", ip="localhost", port=8000, model_name="rednote-hilab/dots.mocr", system_prompt=None,
                    top_logprobs=0, score_eos=True):
    """Score given answers to ONE page in one request: the dots_ocr_amd server's own `score_candidates` field.  Nothing is
    generated; choice i carries candidates[i], its per-token logprobs and their sum.  Returns the choices as dicts in that order, or None on
    a request error.  No sampling field is sent: the server refuses them beside this one."""
    import requests
    from openai import OpenAI        # optional dependency, imported lazily
    client = OpenAI(api_key=os.environ.get("API_KEY", "0"), base_url=f"{protocol}://{ip}:{port}/v1")
    messages = [{"role": "system", "content": system_prompt}] if system_prompt else []
    messages.append({"role": "user", "content": [
        {"type": "image_url", "image_url": {"url": PILimage_to_base64(image)}},
        {"type": "text", "text": f"<|img|><|imgpad|><|endofimg|>{prompt}"}]})
    try:
        r = client.chat.completions.create(messages=messages, model=model_name,
                                           extra_body={"score_candidates": list(candidates), "top_logprobs": int(top_logprobs), "score_eos": bool(score_eos)})
        return [c.model_dump() for c in sorted(r.choices, key=lambda c: c.index)]
    except requests.exceptions.RequestException as e:
        print(f"request error: {e}")
        return None
