"""Reference of the problem-type tests: Hugging Face's ForSequenceClassificationLoss (transformers/loss/loss_utils.py) on
top of given logits, and the trainers' two-phase schedule on oracle.vit_oracle.forward with that loss.

tests/test_problem_type_cpu.py pins `loss` to the `.loss` of the Hugging Face classes; the GPU tests compare the kernels
and the trainers with it.  The loss is computed in the dtype of the logits (float64 logits give the float64 reference of
the kernel tests; the oracle's fp32 logits keep it differentiable for the model tests)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_oracle as vo
from oracle.eegnet_oracle import adam_step_

PROBLEM_TYPES = ("regression", "single_label_classification", "multi_label_classification")


def loss(logits, labels, problem_type):
    """HF's loss for `problem_type` (already resolved), mean reduction."""
    num_labels = logits.shape[-1]
    if problem_type == "regression":
        labels = labels.to(logits.dtype)
        if num_labels == 1:                 # HF squeezes both: [B] and [B, 1] targets are the same thing
            return F.mse_loss(logits.squeeze(), labels.squeeze())
        return F.mse_loss(logits, labels)
    if problem_type == "single_label_classification":
        return F.cross_entropy(logits.view(-1, num_labels), labels.view(-1))
    if problem_type == "multi_label_classification":
        return F.binary_cross_entropy_with_logits(logits, labels.to(logits.dtype))
    raise ValueError(problem_type)


def hf_model(ocfg, problem_type=None):
    """The Hugging Face class of a vit_oracle configuration."""
    from transformers import ASTConfig, ASTForAudioClassification, ViTConfig, ViTForImageClassification
    common = dict(hidden_size=ocfg["hidden"], num_hidden_layers=ocfg["layers"], num_attention_heads=ocfg["heads"],
                  intermediate_size=ocfg["ff"], patch_size=ocfg["patch"], layer_norm_eps=ocfg["eps"],
                  num_labels=ocfg["num_labels"], problem_type=problem_type)
    if ocfg["kind"] == "ast":
        return ASTForAudioClassification(ASTConfig(frequency_stride=ocfg["fstride"], time_stride=ocfg["tstride"],
                                                   max_length=ocfg["frames"], num_mel_bins=ocfg["mel"], **common))
    return ViTForImageClassification(ViTConfig(image_size=ocfg["image"], num_channels=ocfg["channels"], **common))


def step_reference(W, ocfg, x, y, problem_type, freeze):
    """(logits, loss, {name: gradient}) of one labelled forward + backward of the oracle on weights W (numpy, HF names)."""
    hk = set(vo.head_keys(ocfg))
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).clone().requires_grad_((not freeze) or k in hk) for k, v in W.items()}
    logits = vo.forward(P, torch.as_tensor(x), ocfg)
    l = loss(logits, torch.as_tensor(y), problem_type)
    l.backward()
    return logits.detach(), l.detach(), {k: p.grad for k, p in P.items() if p.grad is not None}


class Stepper(vo.Stepper):
    """vo.Stepper with the loss of a problem type: logits -> loss -> backward -> AdamW(wd = 0.01) over the parameters
    that require grad, the body of the trainers' train()."""

    def __init__(self, P, cfg, problem_type, weight_decay=0.01):
        super().__init__(P, cfg, lr=None, weight_decay=weight_decay)
        self.problem_type = problem_type

    def step(self, x, y, freeze, lr):
        hk = set(vo.head_keys(self.cfg))
        for k, p in self.P.items():
            p.grad = None
            p.requires_grad_((not freeze) or (k in hk))
        logits = vo.forward(self.P, x, self.cfg)
        l = loss(logits, y, self.problem_type)
        l.backward()
        with torch.no_grad():
            for k, p in self.P.items():
                if p.grad is None:
                    continue
                self.t[k] += 1
                adam_step_(p, p.grad, self.m[k], self.v[k], self.t[k], lr, weight_decay=self.wd, decoupled=True)
        return logits.detach(), l.detach()

    def predict(self, x, batch):
        with torch.no_grad():
            return torch.cat([vo.forward(self.P, x[i:i + batch], self.cfg) for i in range(0, len(x), batch)]).numpy()


def train_reference(W, ocfg, problem_type, tr_x, tr_y, te_x, phases, batch):
    """The trainers' schedule on the oracle: phases = [(lr, freeze, [epoch orders])]; one AdamW spans the phases (its step
    counts per tensor, like torch's).  Returns the test logits after the last epoch of the last phase."""
    st = Stepper({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in W.items()}, ocfg, problem_type)
    tr_x, tr_y, te_x = torch.as_tensor(tr_x), torch.as_tensor(tr_y), torch.as_tensor(te_x)
    for lr, freeze, orders in phases:
        for order in orders:
            order = [int(i) for i in order]
            for i in range(0, len(order), batch):
                idx = torch.tensor(order[i:i + batch])
                st.step(tr_x[idx], tr_y[idx], freeze, lr)
    return st.predict(te_x, batch), st
