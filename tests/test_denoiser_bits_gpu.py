"""Output bits of the diffusion head's kernels, pinned: SHA-256 of the raw bytes of what
mmt_diffusion_sample_steps, mmt_diffusion_loss_multi, mmt_diffusion_sample, mmt_diffusion_prep and
mmt_head_continuous write, against digests recorded once on an MI355X from a checkout of the commit
before the sampler and the loss kernels were folded onto csrc/denoiser_wave.h (the precedent is
PARENT_LOSS_BITS of tests/test_diffusion_multi_gpu.py). Equality, no tolerance: a refactor of these
kernels that changes one bit of any output (a product contracted differently across a helper
boundary, a sum in another order, a moved draw) fails here, whatever the tolerance tests say.

The cases are the kernel cases of tests/sampler_steps_ref.py and tests/diffusion_multi_ref.py plus
two that reach template instantiations those lists miss: A8 = 4 in the LDS form, and A8 = 6 in the
streamed form (4 * 768 * 56 + 2048 * 12 > 160 KB), the instantiation with the most registers. The
inputs are those files' generators; the two extra loss cases take the generator's first candidate
seed 1000 H + 10 A + B (no tolerance test runs on them, so the pre-activation margin that picks
the seeds of KERNEL_SEEDS does not matter here)."""
import hashlib

import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from tests import diffusion_multi_ref as MR
from tests import heads_chunk_ref as CR
from tests import sampler_steps_ref as SR
from tests import test_diffusion_multi_gpu as TM
from tests import test_heads_chunk_gpu as TH
from tests import test_sampler_steps_gpu as TS

pytestmark = pytest.mark.gpu

EXTRA = [(384, 32, 6, 7), (768, 48, 5, 6)]           # (H, A, B, rows); the loss adds K = 2
STREAMED = [(1024, 64), (768, 48)]                   # (H, A) past the LDS budget
STEP_CASES = SR.KERNEL_CASES + EXTRA
LOSS_CASES = MR.KERNEL_CASES + [c + (2,) for c in EXTRA]
LOSS_OUT = ("loss", "noisy", "h", "dh", "dpred", "dP", "t")
SMALL_STEPS, SMALL_LOSS = SR.KERNEL_CASES[0], MR.KERNEL_CASES[0]   # the rng-driven calls


def sha(t: torch.Tensor) -> str:
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _key(kind, case):
    return kind + "/" + "-".join(str(v) for v in case)


# ------------------------------------------------------------------------------- the calls
def steps_digests(dev, case) -> dict:
    """Injected z: frozen noise, then injected step noise."""
    H, A, B, q_rows = case
    d = TS._dev_inputs(dev, SR.kernel_inputs(H, A, B, q_rows))
    t, coef = (torch.from_numpy(v).to(dev) for v in SR.kernel_table(q_rows))
    out = {}
    for name, fresh in (("frozen", False), ("fresh", True)):
        actions, _, _ = TS._steps(dev, d, A, H, t, coef, 5.0, z_in=d["z"], fresh=fresh,
                                  noise_in=d["noise"] if fresh else None)
        want = (_C.SAMPLER_ROUTE_STEPS_STREAM if (H, A) in STREAMED
                else _C.SAMPLER_ROUTE_STEPS_LDS)
        assert _C.sampler_last_route() == want
        out[name] = sha(actions)
    return out


def steps_rng_digests(dev) -> dict:
    H, A, B, q_rows = SMALL_STEPS
    d = TS._dev_inputs(dev, SR.kernel_inputs(H, A, B, q_rows))
    t, coef = (torch.from_numpy(v).to(dev) for v in SR.kernel_table(q_rows))
    rng = torch.tensor([4321, 9], dtype=torch.int32, device=dev)
    a, z, n = TS._steps(dev, d, A, H, t, coef, 5.0, rng=rng, fresh=True, sample_offset=40,
                        want_z=True, want_noise=True)
    return dict(actions=sha(a), z=sha(z), noise=sha(n))


def _loss_inputs(case):
    seed = None if case in MR.KERNEL_SEEDS else 1000 * case[0] + 10 * case[1] + case[2]
    return MR.kernel_inputs(*case, seed=seed)


def loss_digests(dev, case) -> dict:
    """Injected (t, eps), the random mask, forward and backward."""
    H, A, B, steps, K = case
    inp = _loss_inputs(case)
    d = TM._dev_inputs(dev, inp)
    o = TM._loss(dev, d, case, mask=torch.from_numpy(inp["mask"]).to(dev), grad_scale=float(K * B))
    want = (_C.DIFFUSION_LOSS_ROUTE_STREAM if (H, A) in STREAMED
            else _C.DIFFUSION_LOSS_ROUTE_LDS)
    assert _C.diffusion_loss_last_route() == want
    return {k: sha(o[k]) for k in LOSS_OUT}


def loss_rng_digests(dev) -> dict:
    inp = _loss_inputs(SMALL_LOSS)
    d = TM._dev_inputs(dev, inp)
    rng = torch.tensor([4321, 9], dtype=torch.int32, device=dev)
    o = TM._loss(dev, d, SMALL_LOSS, mask=torch.from_numpy(inp["mask"]).to(dev), rng=rng,
                 inject=False, sample_offset=40)
    return {k: sha(o[k]) for k in LOSS_OUT + ("eps",)}


def prep_digests(dev) -> dict:
    B, A, steps, F = 5, 8, 7, 4
    d = TM._dev_inputs(dev, _loss_inputs(SMALL_LOSS))
    rng = torch.tensor([4321, 9], dtype=torch.int32, device=dev)
    t = torch.empty(B, dtype=torch.int32, device=dev)
    eps = torch.empty((B, A), dtype=torch.float32, device=dev)
    cat = torch.empty((B, A), dtype=torch.bfloat16, device=dev)
    feats = torch.empty((B, 2 * F), dtype=torch.bfloat16, device=dev)
    fw = torch.linspace(0.1, 0.7, F, dtype=torch.float32, device=dev)
    _C.call("mmt_diffusion_prep", _C.ptr(rng), B, A, steps, 40, _C.ptr(d["actions"]),
            _C.ptr(d["alpha_hats"]), _C.ptr(fw), F, None, None, _C.ptr(t), _C.ptr(eps), _C.ptr(cat),
            cat.stride(0), _C.ptr(feats), _C.stream_ptr())
    return dict(t=sha(t), eps=sha(eps), cat=sha(cat), feats=sha(feats))


def legacy_digests(dev) -> dict:
    H, A, B, q_rows = SMALL_STEPS
    d = TS._dev_inputs(dev, SR.kernel_inputs(H, A, B, q_rows))
    rng = torch.tensor([4321, 9], dtype=torch.int32, device=dev)
    coef = torch.tensor([[0.95, 0.2, 0.1]] * q_rows, dtype=torch.float32, device=dev)
    actions = torch.empty((B, A), dtype=torch.float32, device=dev)
    z = torch.empty((B, A), dtype=torch.float32, device=dev)
    _C.call("mmt_diffusion_sample", _C.ptr(rng), B, A, q_rows, 40, _C.ptr(d["P"]), d["P"].stride(0),
            _C.ptr(d["Q"]), d["Q"].stride(0), _C.ptr(d["w1"]), d["w1"].stride(0), _C.ptr(d["w2"]),
            _C.ptr(d["b2"]), _C.ptr(coef), None, H, _C.ptr(actions), _C.ptr(z), _C.stream_ptr())
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_LEGACY_WAVE
    return dict(actions=sha(actions), z=sha(z))


def continuous_digests(dev) -> dict:
    B, h, A = CR.CONT_CASES[1]
    inp = CR.cont_inputs(B, h, A)
    o = TH._cont(dev, inp["z"], inp["y"], inp["mask"], h, A, "mse")
    return {k: sha(o[k]) for k in ("loss", "dz", "pred")}


def all_digests(dev) -> dict:
    """Every pinned digest by key (the recording job prints this from a build of the parent)."""
    out = {_key("steps", c): steps_digests(dev, c) for c in STEP_CASES}
    out.update({_key("loss", c): loss_digests(dev, c) for c in LOSS_CASES})
    out.update({"steps/rng": steps_rng_digests(dev), "loss/rng": loss_rng_digests(dev),
                "prep/rng": prep_digests(dev), "legacy/rng": legacy_digests(dev),
                "continuous": continuous_digests(dev)})
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------- the pins
EXPECTED = {
    "steps/192-8-5-7": {
        "frozen": "ee5de53fb0b44d465a35beb1f1b4c9c5a801652d66ee9cf8a269e5a6f0bba3b8",
        "fresh": "d514344b7ae235fd74475d1ba4b766ed038086729864c6c89d7951722319f42a",
    },
    "steps/200-24-33-12": {
        "frozen": "9e399f351dea5a4219c66ec2dd3c81ac1912f7e143d8b15c13018859189cb91c",
        "fresh": "31a32bc4aeaa5cf0b8baa56c2196239f1eed65a540be0bc29e45be8d4aefc5d7",
    },
    "steps/384-40-70-12": {
        "frozen": "37b92de10661ee05f8fb15e7c76346cc37256ee00999b6c9b3d622bc70bdd0c2",
        "fresh": "b4834bbd4fe29b06e152193d82b6ef94dbd478d4e489474c1a3dd16bad6b5ff2",
    },
    "steps/1024-64-9-5": {
        "frozen": "5dbe6e8e9b59984b697e0b0abd8dedbdd16c12d8efb087513b410d2bb3397124",
        "fresh": "1670af38666061f26dfc9a2671d05777c7f3e36015cf8a361505f82e23049410",
    },
    "steps/384-32-6-7": {
        "frozen": "788b0c3c2f890bf3eee78479eebeb0ea659ef9c896e1941ed9f8247ea45578c5",
        "fresh": "002f9ea3feb01b24e2d2e41bea36a324b62f27a82792738041a438ef6310104a",
    },
    "steps/768-48-5-6": {
        "frozen": "9143060cf8bca61f85fdf18567efd8e1937db20b286c5d85d0ac1672eda283dd",
        "fresh": "87327cc8738bd942b5bbc0d73af0df08d12f0816a5baa3bb55f12b835213277e",
    },
    "loss/192-8-5-7-3": {
        "loss": "139f92faeb99456d0491a1a313b1a8bac4504264d596a96aa365f44e45429372",
        "noisy": "22ab99118faa841a45cef11c1fed04a44f1a3caedc586231b18cbf46fe3e656d",
        "h": "19e123986318e8acc682916f6609fe8eced22b2e63d74cf3a7b7c982fb072a42",
        "dh": "cf93643b6ae254960e636c2ee57ab26e4a2465f13120d065ddfe40a4a5fa80e1",
        "dpred": "d11fbe02a14d76e08ea3fd51c97708f43804c131bb487f68680390985bd82caa",
        "dP": "31d52dd4148966984f60c7379469599ababd8e3a8a349239967bd779cc566367",
        "t": "2113fc093a48bfaf3ae61216ee2187f96b7c9fb63fdd974813eb464f4db59398",
    },
    "loss/200-24-33-12-2": {
        "loss": "7318b248b8b222c00ff744b9bc8a22a2582ce08e6b7bda52fed26fc08616ba81",
        "noisy": "1ed8820cb356c39369e8ae95a74d09775858b91f8f572e4e632e00c32e16a547",
        "h": "086f5b0e2bb889ad36eb2c44e3dd6cc753b8ec21be53c5d2e3476210beeb498a",
        "dh": "1acbb19ae44a9895fa19e1a265f6e860a2ce1423acc3f78ae945b32607b3ef20",
        "dpred": "449cba9bddcb80538fd1c2eb8dd1f86121b4a8a07ea43634d8b0e31cc14003e0",
        "dP": "dba8f1105bb368719a0be72c1d43245b380508953abcc49d9bf3e5b63a1fdb42",
        "t": "0d965d3d567fa5ff8e144962ab018db3332240185ae499d98398e97a65e17d98",
    },
    "loss/384-40-18-12-4": {
        "loss": "3f6f257f35c429c7a159ed6af571eafe6e64236e1a31ba1d1e2ef8c38679f823",
        "noisy": "618538d906a8d7470d50779a1d87cc32907a677256cc4a9434ad4528d2b9e688",
        "h": "ca248aa71b0a88d3edb9ba30882aecf62a013603d0498bfab5f823e85713a9d3",
        "dh": "a6c9b82168a542f1bfc965822d5968d1bf48d8632096f832936fdbb9a11e4228",
        "dpred": "f1c8c127650af00d1b9837e0fd933ac913613d33d0d44136d0dadd6f22c8d7ed",
        "dP": "4ca6e219bbe09643c6a6f47f92bb941f0376a26aeda5389e19ec9b72d2c24444",
        "t": "b55d992c262f0d3acb79d4794bbdda35e74cda3783831ee672a575f1f4d2272c",
    },
    "loss/1024-64-9-5-2": {
        "loss": "6fc8c28d54426cb8937f3d494bac2e3773db82ae594b7e7991c1cdce47bff8b7",
        "noisy": "23c0f4dd592887ffa0054f072dd94683c0a39cbea12fcc4a1f3ef02997d2085c",
        "h": "91ebf7628ca2f9a27fc188166079e69624ea9d5bf062362f0054eeb4f484be7a",
        "dh": "7d1143bfd18c1b86aa038e8ee6edfab1b07084ba305005af76ce42d2ebf2e0bb",
        "dpred": "11801710fa7084a2df5706365e5ffa960264e2f90dea1f1e16884b74bc5c31d4",
        "dP": "132ef859e245c5b3e5414100a207a9e8e8605127bb2d005ab16ac2a93ff4b1f8",
        "t": "109cf24ef5e40c75e2d0b17c0d13272f24bcfeca76c352335289c8fec7f80f1d",
    },
    "loss/64-16-4-32-1": {
        "loss": "a8713b31725a1dd6ba794c218cf1755d70487cfb0cb9b54972b26a622746c0e6",
        "noisy": "37e74782b67708ab115c61e352b1f50523f940769c8ab51ed7069d2e4e8332cc",
        "h": "fb076c4dbb14131a95829e1b473f56bc5e9b556c7f79086041bd40af86dd9639",
        "dh": "e55aab13453652bc3b5815dd15a56db34f8c2a557f958a67895ec207f73d9f54",
        "dpred": "7876c29f54bc038c33e2d8ca74a83ba05cbb4a00d7587e0ae0632e89eb31ddef",
        "dP": "e55aab13453652bc3b5815dd15a56db34f8c2a557f958a67895ec207f73d9f54",
        "t": "0962d9877d70cf852d1db24e68c4cc7711107a5bb389f48a9fc5f7dd70977aa5",
    },
    "loss/384-32-6-7-2": {
        "loss": "ceba62642d57f382f49451a3a960f66b3a193d9e83a693a159b8f0c9c99dcdeb",
        "noisy": "61dc933fe0fe07ebea04393dc0ca3417a7099ddf310a50ecef732c5ac8b7cf81",
        "h": "99cb327bf378bbd8ca5d04b2f046a3bddebe94813bad6280a5cb1e1fe34a36e3",
        "dh": "e4d7c764d8d5ab11a6e9f05584489ae8d883600fb7dd7ab7cb59bc4d0d74f9f3",
        "dpred": "8141e7867330cefdd8f06da2da097ff281690a0587452f4740aac8895775f322",
        "dP": "624b1e9b6f893ef1a35116f896d95cedd83ccc8e8c30216157e1da3ae90f40d5",
        "t": "9dfdcfaf934acae80b74baace8c04b3addfd984a37ff914b8097e82ac6527e2a",
    },
    "loss/768-48-5-6-2": {
        "loss": "69bf3756a4d311dae0293d215a21c060f8bde8a4c973c786dbd53ee92b4e36c3",
        "noisy": "81993a1b22f1209bc885ae317fd49f9ec9d082561cf095c50235822e689510b4",
        "h": "132939a615037bfedfe712ce1d52895e8a031a4d516e771688cb7e414236d17d",
        "dh": "3f97fc87adf4cf36d7bbdf92fc0de3b04cd4569615ab814ab73207bce7a85d7d",
        "dpred": "35fd99bee8125abb072c4a24600f695e83f1bbec326329cb75d62c9457066aed",
        "dP": "5518867c3b014aaf0ed2a802ed33f28a2e6e562220fa6c1807aa30dd38da8edd",
        "t": "93bb29b93315f620904b02a3e6f04a39e242d4fc49aa723349c4235d03324f4f",
    },
    "steps/rng": {
        "actions": "350931d619a1478b971e9d8efdad86f21877f1b68b928d6b653cf1f599e2e28f",
        "z": "ec7688f47e939c6e699df843bd1de76893d9a60878239ba95ea0447ac1c82bb8",
        "noise": "5419cc8df1bbef175aeba990d4f68a3c9926181dcd0e3bf0fd1fe7b627eccd28",
    },
    "loss/rng": {
        "loss": "647c5a88a726917e08a8a9489f1a464ca5c7589fbec020c4d09bff69cc007a1c",
        "noisy": "4a266184f1f934c9344ace5de931442139faf2f5f2ccd7c2d36fdbd5ebf2fd2f",
        "h": "af5cdab256033b0068f9c1705606be6c105b28110d8400b34b13ddec363e8f73",
        "dh": "fe11f28e2d817c853e826e67880e8b3735dd6ea1d9e656af75523bbf313e5785",
        "dpred": "519653a97ed1862669c74a18942e4047d9246ed4417dfc1556db4c562e4d3eb0",
        "dP": "83eed586346a6573267e770529e42a9ec6a7c06e54551065852ac0eeba9da3cf",
        "t": "492b01171e3a96405615334c682153a72e5aa8f2a6d68533dbe60a346d251345",
        "eps": "48816bcd2fee3dc1637f1bf21329b928bc0add1a26e3a66279ec802420caf582",
    },
    "prep/rng": {
        "t": "7fa9df86b92c6eef609ad85905c35ac0598acc10fb2283c0002cc627e75bf308",
        "eps": "8335c95d211d95d529ff57beab9ab3925af3709891a2df8b60397faf1de2e548",
        "cat": "1e4e8476c975e3dd91d1da1bae9fef143eb52d31c1ad2724a8dffdc46be191c0",
        "feats": "bbd6eb34874e9de353b55e71a1ab74cedc8cf808e65481e188b091bdaa603caf",
    },
    "legacy/rng": {
        "actions": "2a65c7b81b232fbe003769b83403b8d3c415b1491e28fe56924283dadba34e45",
        "z": "ec7688f47e939c6e699df843bd1de76893d9a60878239ba95ea0447ac1c82bb8",
    },
    "continuous": {
        "loss": "2aa9ac3f44eb1e01609191b1a3cab3e9f5408465c634c5eb2a8b004d610ce8c8",
        "dz": "c905ca4c49f24ded83025616593a754d5ee4e216948d37317cf073ddb1097cb8",
        "pred": "f9225b6ec08b5ec100c8cf97bbc0049319b97fea6cbb516bfb89f099fc918213",
    },
}


def _pinned(key, got):
    print(key, got)
    assert got == EXPECTED[key], key


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "H%d-A%d-B%d-q%d" % c)
def test_step_sampler_bits(dev, case):
    _pinned(_key("steps", case), steps_digests(dev, case))


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "H%d-A%d-B%d-S%d-K%d" % c)
def test_loss_bits(dev, case):
    _pinned(_key("loss", case), loss_digests(dev, case))


@pytest.mark.parametrize("key,fn", [("steps/rng", steps_rng_digests), ("loss/rng", loss_rng_digests),
                                    ("prep/rng", prep_digests), ("legacy/rng", legacy_digests),
                                    ("continuous", continuous_digests)],
                         ids=["steps", "loss", "prep", "legacy", "continuous"])
def test_drawn_and_neighbouring_bits(dev, key, fn):
    """One rng-driven call of each kernel that draws (the step sampler and the loss at their
    smallest case, the single-draw prep kernel, the register-resident sampler) and the continuous
    head with a random mask (its mask count is shared with the loss)."""
    _pinned(key, fn(dev))
    _C.call("mmt_device_status", _C.stream_ptr())
