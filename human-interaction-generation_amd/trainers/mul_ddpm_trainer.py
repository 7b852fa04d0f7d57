"""MI355X-native `DDPMMulTrainer`: the reference's two-person trainer
(codes/trainers/mul_ddpm_trainer.py:51-440) over the HIP two-person denoiser.

Batch layouts (reference :96-131).  With a label file: model batch = [m1 | m2] with captions
[c1 | c2].  Without one (PIT, permutation-invariant training): the noised motions are run twice,
[m1, m1 | m2, m2] with captions [c1, c2 | c2, c1], and per pair the cheaper caption assignment is
the loss (:234-243).  `multi=False` falls back to the single-person trainer's step.
"""
import os
from collections import Counter, OrderedDict

import numpy as np
import torch

from .. import _lib
from .ddpm_trainer import DDPMTrainer, _core


LABEL_STEPS = range(830, 940, 30)      # the four timesteps of the reference's labelling pass (mul_ddpm_trainer.py:411, 430)


def label_pass_option(opt):
    """opt.label_pass: "torch" (the default: `eval_data` loops over `label_batch`, as the reference) or "hip" (one
    `label_votes` call per batch).  Anything else is a ValueError."""
    v = getattr(opt, "label_pass", "torch")
    if v not in ("torch", "hip"):
        raise ValueError("opt.label_pass must be 'torch' or 'hip' (got %r)" % (v,))
    return v


def _most_common(first_value, counts):
    """`Counter(values).most_common()[0][0]` from the counts and the value inserted first: most_common sorts by count with a
    stable sort over insertion order, so among equal counts the value inserted first wins."""
    best = first_value
    for value, n in counts.items():
        if n > counts[best]:
            best = value
    return best


def learned_indices_from_votes(batches, max_class_num=42):
    """Model mode of `eval_data` (mul_ddpm_trainer.py:405-425 of the reference) from per-batch votes.

    batches: [(ids1, ids2, votes (steps, pairs, 2), first (pairs,)), ...] in the loader's order, as `label_votes` returns them
    (assignment 0 keeps the caption order 'a_b', assignment 1 swaps it to 'b_a').  Returns `learned_indices`.

    The reference merges one list per pair key 'a_b', appending timestep-outer, batch-inner, draw, pair, and takes
    `Counter(list).most_common()[0][0]`: the larger count, and on a tie the value that entered the list first.  The counts do
    not depend on the order, so they are the sums of `votes` over steps, batches and the pairs that carry the key.  The value
    that entered first is reconstructed: the reference's first visit of a key is at the FIRST timestep (every batch is visited
    under it before the second timestep starts), in the first batch of the loader that holds the key, at its first draw, at the
    lowest pair index with that key -- and that draw's decision is `first[p]` of that batch, because `label_votes` casts the
    first vote of every pair at steps[0], draw 0.  Being batch-outer here therefore changes nothing the winner depends on."""
    counts, first_value = {}, {}
    for ids1, ids2, votes, first in batches:
        votes = np.asarray(votes).reshape(-1, len(ids1), 2).sum(axis=0)
        for p, (a, b) in enumerate(zip(ids1, ids2)):
            a, b = int(a), int(b)
            key, values = '%d_%d' % (a, b), ('%d_%d' % (a, b), '%d_%d' % (b, a))
            c = counts.setdefault(key, {})
            if key not in first_value:
                first_value[key] = values[int(first[p])]
                c[first_value[key]] = 0
            for a_, n in zip(values, votes[p]):
                if int(n):
                    c[a_] = c.get(a_, 0) + int(n)
    learned_indices = []
    for i in range(max_class_num + 1):
        if '%d_%d' % (i - 1, i) in counts:
            continue
        key = '%d_%d' % (i, i + 1)
        if key in counts:
            num1, num2 = _most_common(first_value[key], counts[key]).split('_')
            learned_indices += [int(num1), int(num2)]
        else:
            learned_indices.append(i)
    return learned_indices


def label_active_indices(learned_indices, ids1, ids2):
    """Which caption of each pair the learned order puts first (label_batch: argmin over the two learned positions)."""
    return np.argmin([[learned_indices[int(c)] for c in ids1], [learned_indices[int(c)] for c in ids2]], axis=0)


def file_labels_from_votes(file_ids, active_indices, votes, first):
    """Label mode of `eval_data` (mul_ddpm_trainer.py:427-440 of the reference) for one batch: {file id: 0 or 1} in the order
    the reference's dictionary has.  A draw's output for pair p is 0 where its assignment equals active_indices[p], else 1;
    a file's label is `Counter(outputs).most_common()[0][0]` over steps x draws: the larger count, a tie going to the output
    of the first draw -- first[p] against active_indices[p], at the lowest pair index that carries the file id."""
    votes = np.asarray(votes).reshape(-1, len(file_ids), 2).sum(axis=0)
    counts, first_value = OrderedDict(), {}
    for p, fid in enumerate(file_ids):
        act = int(active_indices[p])
        c = counts.setdefault(fid, {})
        if fid not in first_value:
            first_value[fid] = 0 if int(first[p]) == act else 1
            c[first_value[fid]] = 0
        for a, n in enumerate(votes[p]):
            if int(n):
                out = 0 if a == act else 1
                c[out] = c.get(out, 0) + int(n)
    return OrderedDict((fid, _most_common(first_value[fid], c)) for fid, c in counts.items())


class DDPMMulTrainer(DDPMTrainer):

    def __init__(self, args, encoder):
        super().__init__(args, encoder)
        self.multi = args.multi
        self.with_label = args.label_path is not None
        self.cap_id = args.cap_id
        label_pass_option(args)        # (a bad opt.label_pass is refused here, not at the first eval_data)

    # ---- one training forward ---------------------------------------------------------------
    def _pair_inputs(self, batch_data):
        caption1, caption2, motion1, motion2, m_lens = batch_data[:5]
        motion1 = motion1.detach().to(self.device).float()
        motion2 = motion2.detach().to(self.device).float()
        x_start = torch.cat([motion1, motion2], dim=0)
        caption = list(caption1) + list(caption2)
        T = x_start.shape[1]
        cur_len = torch.LongTensor([min(T, int(m_len)) for m_len in m_lens]).to(self.device)
        return caption, list(caption1), list(caption2), x_start, cur_len, motion1.shape[0], T

    def _drop_pair_captions(self, caption1, caption2):
        """Caption dropout per PAIR: one draw blanks both captions of a pair, in every ordering the PIT loss builds from them."""
        keep = self._caption_keep(len(caption1))
        if keep is None:
            return caption1, caption2
        return ([c if k else "" for c, k in zip(caption1, keep)], [c if k else "" for c, k in zip(caption2, keep)])

    def _guidance_group(self, B):
        return B // 2 if self.multi else B

    def forward(self, batch_data, eval_mode=False):
        """mul_ddpm_trainer.py:90-161."""
        if not self.multi:
            return super().forward(batch_data, eval_mode)
        caption, caption1, caption2, x_start, cur_len, B, T = self._pair_inputs(batch_data)
        caption1, caption2 = self._drop_pair_captions(caption1, caption2)
        caption = caption1 + caption2
        t = self._draw_t(B, x_start.device)
        t = self._t = torch.cat([t, t], dim=0)
        if not self.with_label:
            caption = caption + caption2 + caption1      # (c1, c2, c2, c1) against (m1, m1, m2, m2)
            cur_len = torch.cat([cur_len] * 4, dim=0)
            forward_twice = True
        else:
            cur_len = torch.cat([cur_len, cur_len], dim=0)
            forward_twice = False
        output = self.diffusion.training_losses(
            model=self.encoder, x_start=x_start, t=t,
            model_kwargs={"text": caption, "length": cur_len}, forward_twice=forward_twice)
        self.real_noise = output['target']
        self.fake_noise = output['pred']
        self.src_mask = _core(self.encoder).generate_src_mask(T, cur_len).to(x_start.device)

    def _token_loss(self):
        """(rows, T) per-token MSE; the init-pose token is scored on its 4 features (:226-228)."""
        init = self.mse_criterion(self.fake_noise[:, 0, :4], self.real_noise[:, 0, :4]).mean(dim=-1)
        move = self.mse_criterion(self.fake_noise[:, 1:], self.real_noise[:, 1:]).mean(dim=-1)
        return torch.cat([init.unsqueeze(1), move], dim=1)

    def backward_G(self):
        """mul_ddpm_trainer.py:223-249."""
        if not self.multi:
            return super().backward_G()
        if self._loss_cfg[0] is not None or self._loss_cfg[2] != "uniform":
            return self._backward_G_weighted()
        if self.with_label:
            if _core(self.encoder).two_embed:
                loss = self._token_loss()
            else:
                loss = self.mse_criterion(self.fake_noise, self.real_noise).mean(dim=-1)
            loss_mot_rec = (loss * self.src_mask).sum() / self.src_mask.sum()
        else:
            loss = self._token_loss()
            rows = loss.shape[0]
            # per caption assignment: person-1 rows + person-2 rows  -> (2 assignments x pairs)
            per_assign = (loss * self.src_mask).sum(dim=1).view(2, rows // 2).sum(dim=0)
            loss_mot_rec = per_assign.view(2, rows // 4).min(dim=0).values.sum() / (self.src_mask.sum() / 2)
        self.loss_mot_rec = loss_mot_rec
        return OrderedDict({'loss_mot_rec': self.loss_mot_rec.item()})

    def _backward_G_weighted(self):
        """backward_G under opt.loss_weighting / opt.sampler: what hig_pair_mse_w computes.  Labelled: row r counts w[t_r]
        times.  PIT: the assignment is chosen on the unweighted sums, the chosen sum of pair p counts w[t_p] times."""
        mask = self.src_mask
        if self.with_label:
            loss = self._token_loss() if _core(self.encoder).two_embed else self.mse_criterion(self.fake_noise, self.real_noise).mean(dim=-1)
            self.loss_mot_rec = self._weighted((loss * mask).sum(dim=1), mask.sum(), self._t, mask.sum(dim=1).clamp_min(1), loss.device)
        else:
            loss = self._token_loss()
            rows = loss.shape[0]
            per_assign = (loss * mask).sum(dim=1).view(2, rows // 2).sum(dim=0)
            chosen = per_assign.view(2, rows // 4).min(dim=0).values
            self.loss_mot_rec = self._weighted(chosen, mask.sum() / 2, self._t, 2 * mask[:rows // 4].sum(dim=1).clamp_min(1), loss.device)
        return OrderedDict({'loss_mot_rec': self.loss_mot_rec.item()})

    # ---- MI355X fused step (inherits train_step_fused / train_step_captured) ---------------------
    def _denoise_loss_backward(self, x_start, t, length, xf_proj, xf_out, noise, exchange):
        """Two-person middle of the fused forward/backward: x_start = cat([motion1, motion2]) (2B, T, F),
        t (B,) or (2B,), length (B,) per pair.  PIT mode (no label file): the noised motions run twice,
        rows [m1|c1, m1|c2, m2|c2, m2|c1] -- xf_proj / xf_out must hold the 4B text embeddings in that
        order (2B rows [c1 | c2] with a label file) -- and `hig_pair_mse` picks the cheaper caption
        assignment per pair (mul_ddpm_trainer.py:96-131, 223-247).  Whatever the step's text source is (CLIP features, a
        CaptionBatch -- half of the 4B PIT rows are duplicates by construction -- or class ids), it covers those rows."""
        if not self.multi:
            return super()._denoise_loss_backward(x_start, t, length, xf_proj, xf_out, noise, exchange)
        core = _core(self.encoder)
        st = self.fused_state()
        B2, T, F = x_start.shape
        B = B2 // 2
        t2 = t if t.numel() == B2 else torch.cat([t, t])
        if noise is None:
            noise = torch.randn_like(x_start)
        x_t = self.diffusion.q_sample(x_start, t2, noise=noise)
        pit = not self.with_label
        if pit:   # gaussian_diffusion.py:996-1001 (forward_twice)
            x_t = torch.cat([x_t[:B], x_t[:B], x_t[B:], x_t[B:]])
            noise = torch.cat([noise[:B], noise[:B], noise[B:], noise[B:]])
            t2 = torch.cat([t2, t2])
        rows = x_t.shape[0]
        len_rows = torch.cat([length] * (rows // B)).contiguous()
        assert xf_proj.shape[0] == rows and xf_out.shape[0] == rows, "text embeddings must cover the model batch"
        pred, saved = core._launch_forward(x_t, t2, len_rows, xf_proj, xf_out, training=True)
        dpred = torch.empty_like(pred)
        scr = self._loss_buffer(st, "pair_scratch", 2 * rows, pred.device)      # (one per size: captured graphs keep theirs)
        wtab, smp = self._loss_state(pred.device)
        if wtab is None:
            _lib.api.hig_pair_mse(pred, noise.contiguous(), len_rows, rows, T, F, pit, st["loss"], dpred, scr)
        else:   # the weighted twin (row r counts w[t2[r]] times); loss-aware: one loss per pair (PIT) or per row, pushed under
            # the first entries of t2, behind the loss launch
            t2 = t2.contiguous()
            sl = None if smp is None else self._loss_buffer(st, "sample_loss", rows // 4 if pit else rows, pred.device)
            _lib.api.hig_pair_mse_w(pred, noise.contiguous(), len_rows, t2, wtab, wtab.numel(), rows, T, F, pit, st["loss"], dpred, sl, scr)
            if smp is not None:
                smp.update(t2, sl)
        hook = {} if exchange is None else dict(layer_hook=exchange.layer_done, comm_stream=exchange.stream)
        _, dxp, dxo = core._launch_backward(x_t, t2, len_rows, xf_out, saved, dpred, want_dx=False, **hook)
        return dxp, dxo

    def train_fused_batch(self, batch_data, captured=False, noise=None):
        """forward(batch) + update() of the reference (mul_ddpm_trainer.py:90-161, 251-258) as one fused step."""
        if not self.multi:
            return super().train_fused_batch(batch_data, captured, noise)
        caption, caption1, caption2, x_start, cur_len, B, T = self._pair_inputs(batch_data)
        caption1, caption2 = self._drop_pair_captions(caption1, caption2)
        caption = caption1 + caption2
        if not self.with_label:
            caption = caption + caption2 + caption1
        t = self._draw_t(B, x_start.device)
        step = self.train_step_captured if captured else self.train_step_fused
        if self.cap_id:
            if not _core(self.encoder)._has_hip_class_head():
                raise NotImplementedError("cap_id models take class embeddings, not the text head: use forward()/update()")
            # the captions are class-id tensors (get_class_embedding's torch.cat), here in the model batch's row order;
            # converted on the host, so the step's only text input is one int32 copy
            ids = torch.cat([torch.as_tensor(c).reshape(-1).cpu() for c in caption]).to(torch.int32).to(self.device)
            return step(x_start.contiguous(), t, cur_len, noise=noise, class_ids=ids)
        return step(x_start.contiguous(), t, cur_len, noise=noise, **self._text_inputs(caption))

    # ---- sampling ---------------------------------------------------------------------------
    def generate_batch(self, caption1, caption2, m_lens, dim_pose, known=None, known_mask=None):
        """mul_ddpm_trainer.py:163-199.  known + known_mask: (2, pairs, T, F) (person, pair), or already in the model batch's
        layout (2 pairs, T, F) = person 1 of all pairs, then person 2; cut to this chunk's T."""
        m_lens = torch.cat([m_lens, m_lens], dim=0)
        core = _core(self.encoder)
        T = min(int(m_lens.max()), core.num_frames)
        if known is not None and known_mask is not None:
            known = torch.as_tensor(known)
            known_mask = torch.broadcast_to(torch.as_tensor(known_mask), known.shape)
            if known.dim() == 4:
                known, known_mask = known.flatten(0, 1), known_mask.flatten(0, 1)
        known, known_mask = self._known_for(known, known_mask, T)
        if self.cap_id:
            caption = [torch.as_tensor(caption1).view(-1), torch.as_tensor(caption2).view(-1)]
            B = len(caption1) + len(caption2)
            kwargs = {'text': caption, 'length': m_lens}
        else:
            caption = list(caption1) + list(caption2)
            B = len(caption)
            xf_proj, xf_out = core.encode_text(caption, self.device)
            kwargs = {'xf_proj': xf_proj, 'xf_out': xf_out, 'length': m_lens}
        return self._sample_loop((B, T, dim_pose), kwargs, known, known_mask)

    def generate(self, caption1, caption2, m_lens, dim_pose, batch_size=512, known=None, known_mask=None):
        """mul_ddpm_trainer.py:201-221 -> list of [motion1, motion2] per pair.  known + known_mask: (2, N, T, F) (person,
        pair), sliced per chunk.  Reaction generation: known[0] = person 1's motion, known_mask[0] = frames < length,
        known_mask[1] = 0."""
        N = len(caption1)
        if known is not None and known_mask is not None:
            known = torch.as_tensor(known)
            known_mask = torch.broadcast_to(torch.as_tensor(known_mask), known.shape)
        cur_idx = 0
        self.encoder.eval()
        all_output = []
        with self._sampling_weights():      # set_sampler(weights="ema"): one exchange around all the chunks
            while cur_idx < N:
                end = N if cur_idx + batch_size >= N else cur_idx + batch_size
                batch_caption1 = caption1[cur_idx:end]
                # the reference slices caption1 again for the second person of a non-final chunk (:212);
                # kept, so chunked generation gives the same conditioning as upstream
                batch_caption2 = caption2[cur_idx:] if end == N else caption1[cur_idx:end]
                batch_m_lens = m_lens[cur_idx:end]
                k = known if known is None else known[:, cur_idx:end]
                km = known_mask if known_mask is None or known is None else known_mask[:, cur_idx:end]
                output = self.generate_batch(batch_caption1, batch_caption2, batch_m_lens, dim_pose, known=k, known_mask=km)
                B = len(batch_caption1)
                motion1, motion2 = output[:B], output[B:]
                for i in range(B):
                    all_output.append([motion1[i], motion2[i]])
                cur_idx += batch_size
        return all_output

    # ---- pseudo-labelling of the caption order (:313-440) --------------------------------------
    def label_batch(self, batch_data, learned_indices, t, label_mode=False):
        caption1, caption2 = batch_data[0], batch_data[1]
        file_id = batch_data[5]
        if learned_indices is not None:
            cap1 = [learned_indices[cap] for cap in caption1[0].numpy()]
            cap2 = [learned_indices[cap] for cap in caption2[0].numpy()]
            active_indices = np.argmin([cap1, cap2], axis=0)
        caption, c1, c2, x_start, cur_len, B, T = self._pair_inputs(batch_data)
        caption = caption + c2 + c1
        tt = torch.full((2 * B,), int(t), dtype=torch.long, device=x_start.device)
        cur_len = torch.cat([cur_len] * 4, dim=0)
        output = self.diffusion.training_losses(
            model=self.encoder, x_start=x_start, t=tt,
            model_kwargs={"text": caption, "length": cur_len}, forward_twice=True)
        self.real_noise = output['target']
        self.fake_noise = output['pred']
        self.src_mask = _core(self.encoder).generate_src_mask(T, cur_len).to(x_start.device)
        loss = self._token_loss()
        rows = loss.shape[0]
        per_assign = (loss * self.src_mask).sum(dim=1).view(2, rows // 2).sum(dim=0).view(2, rows // 4)
        result = per_assign.min(dim=0).indices.cpu().numpy()
        if learned_indices is not None:
            outs = [0 if int(res) == int(active_indices[i]) else 1 for i, res in enumerate(result)]
            return (outs, file_id) if label_mode else np.array(outs)
        active_list = {}
        ids1, ids2 = caption1[0].numpy(), caption2[0].numpy()
        for i, res in enumerate(result):
            a, b = int(ids1[i]), int(ids2[i])
            pair_key = '%d_%d' % (a, b)
            active_list.setdefault(pair_key, []).append('%d_%d' % ((a, b) if res == 0 else (b, a)))
        return active_list

    def label_votes(self, batch_data, steps=LABEL_STEPS, draws=41, noise=None, captured=True, losses=False):
        """The votes `label_batch` would cast for one batch over `steps` x `draws` noise draws, with everything that does not
        change between draws done once: -> dict(votes=int array (len(steps), pairs, 2), first=int array (pairs,)); votes[s, p, a]
        counts the draws at steps[s] in which pair p scored caption assignment a cheaper (0: [c1, c2] as given, 1: swapped; a
        tie is 0), first[p] is the assignment of the very first draw (steps[0], draw 0) -- what Counter's tie rule needs.

        Once per batch: `_pair_inputs`, the ids (train_fused_batch's conversion) or captions, the text embeddings of the 4 pairs
        rows [c1, c2, c2, c1] (hig_class_head_fwd for a class_head="hip" model, get_class_embedding otherwise, encode_text for a
        caption model), the text context (the inference forward's cache), the lengths and the `t` buffers.  One step,
            z.normal_() -> hig_q_sample_pit -> _launch_forward(training=False) at 4 pairs rows -> hig_pair_vote,
        is warmed up on a side stream, captured (captured=True) and replayed `draws` times per timestep; between timesteps the
        host refills the `t` buffers the graph reads.  The host reads `votes` once per timestep (a step's votes are the
        difference of consecutive readings) and checks that every pair gained exactly `draws`: a pair whose loss is NaN casts
        no vote, and the call raises naming it.  captured=False runs the same launches eagerly.

        noise (len(steps), draws, 2 pairs, T, F) replaces the draws (copied into z before each step).  losses=True adds
        `assign_loss` (len(steps), draws, 2, pairs), the two assignment sums of every draw, kept on the device until the end."""
        if not self.multi:
            raise RuntimeError("label_votes: the labelling pass belongs to the two-person trainer (opt.multi)")
        steps, draws = [int(t) for t in steps], int(draws)
        if not steps or draws <= 0:
            raise ValueError("label_votes: at least one timestep and one draw")
        core = _core(self.encoder)
        K = self.diffusion.num_timesteps
        if any(not 0 <= t < K for t in steps):
            raise ValueError("label_votes: steps must lie in [0, %d)" % K)
        assert not self.diffusion.rescale_timesteps
        with torch.no_grad():
            caption, c1, c2, x_start, cur_len, B, T = self._pair_inputs(batch_data)
            caption = caption + c2 + c1                     # (c1, c2, c2, c1) against (m1, m1, m2, m2)
            x_start = x_start.contiguous()
            dev, F = x_start.device, x_start.shape[2]
            if self.cap_id:
                ids = torch.cat([torch.as_tensor(c).reshape(-1).cpu() for c in caption]).to(torch.int32).to(dev)
                if core._has_hip_class_head():
                    xf_proj, xf_out = core._launch_class_head(ids)
                else:
                    xf_proj, xf_out = core.get_class_embedding([ids.long()])
            else:
                xf_proj, xf_out = core.encode_text(caption, dev)
            xf_proj, xf_out = xf_proj.detach().float().contiguous(), xf_out.detach().float().contiguous()
            len4 = torch.cat([cur_len] * 4).contiguous()
            t2 = torch.full((2 * B,), steps[0], dtype=torch.int64, device=dev)
            t4 = torch.full((4 * B,), steps[0], dtype=torch.int64, device=dev)
            z = torch.zeros_like(x_start)
            xt4 = torch.empty(4 * B, T, F, device=dev, dtype=torch.float32)
            votes = torch.zeros(B, 2, dtype=torch.int32, device=dev)
            first = torch.full((B,), -1, dtype=torch.int32, device=dev)
            assign = torch.zeros(2, B, dtype=torch.float32, device=dev)
            scratch = torch.zeros(4 * B, dtype=torch.float32, device=dev)
            tab = self.diffusion.device_table(dev)
            if noise is not None:
                noise = torch.as_tensor(noise)
                if tuple(noise.shape) != (len(steps), draws, 2 * B, T, F):
                    raise ValueError("label_votes: noise must have shape %s, got %s"
                                     % ((len(steps), draws, 2 * B, T, F), tuple(noise.shape)))
                noise = noise.to(dev).float()
                z.copy_(noise[0, 0])
            kept = torch.zeros(len(steps), draws, 2, B, dtype=torch.float32, device=dev) if losses else None

            def step():
                if noise is None:
                    z.normal_()
                _lib.api.hig_q_sample_pit(x_start, z, t2, tab, K, B, T * F, xt4)
                pred, _ = core._launch_forward(xt4, t4, len4, xf_proj, xf_out, training=False)
                _lib.api.hig_pair_vote(pred, z, len4, 4 * B, T, F, votes, first, assign, scratch)

            run = step
            if captured:    # warm-up on a side stream (allocations, text context), then undo its vote
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    step()
                torch.cuda.current_stream().wait_stream(s)
                votes.zero_()
                first.fill_(-1)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    step()
                run = graph.replay
            out = np.zeros((len(steps), B, 2), dtype=np.int64)
            seen = np.zeros((B, 2), dtype=np.int64)
            for si, t in enumerate(steps):
                t2.fill_(t)
                t4.fill_(t)
                for d in range(draws):
                    if noise is not None:
                        z.copy_(noise[si, d])
                    run()
                    if losses:
                        kept[si, d].copy_(assign)
                now = votes.cpu().numpy().astype(np.int64)
                out[si] = now - seen
                seen = now
                short = np.nonzero(out[si].sum(axis=1) != draws)[0]
                if short.size:
                    raise RuntimeError("label_votes: pair %d of the batch cast %d of %d votes at t = %d: its loss is NaN "
                                       "(pairs %s)" % (short[0], out[si, short[0]].sum(), draws, t, short.tolist()))
            result = dict(votes=out, first=first.cpu().numpy().astype(np.int64))
            if losses:
                result["assign_loss"] = kept.cpu().numpy()
        return result

    def _eval_data_votes(self, loader, learned_indices, max_class_num, save_dir):
        """`eval_data` under opt.label_pass == "hip": one `label_votes` call per batch, then the reference's bookkeeping as
        pure host functions of the votes."""
        if learned_indices is None:
            batches = []
            for batch_data in loader:
                r = self.label_votes(batch_data, LABEL_STEPS, draws=5)
                batches.append((batch_data[0][0].numpy(), batch_data[1][0].numpy(), r["votes"], r["first"]))
            return learned_indices_from_votes(batches, max_class_num)
        for batch_data in loader:
            r = self.label_votes(batch_data, LABEL_STEPS, draws=41)
            active = label_active_indices(learned_indices, batch_data[0][0].numpy(), batch_data[1][0].numpy())
            for key, label in file_labels_from_votes(list(batch_data[5]), active, r["votes"], r["first"]).items():
                with open(os.path.join(save_dir, key + '.txt'), 'w') as f:
                    f.write(str(label))

    def eval_data(self, train_dataset, rank, world_size, learned_indices, max_class_num=42, save_dir=None):
        from ..parallel import ShardedSampler
        self.to(self.device)
        sampler = ShardedSampler(len(train_dataset), rank, world_size, shuffle=False)
        loader = torch.utils.data.DataLoader(train_dataset, batch_size=self.opt.batch_size, sampler=sampler,
                                             drop_last=False, num_workers=getattr(self.opt, "num_workers", 4))
        self.eval_mode()
        if label_pass_option(self.opt) == "hip":
            return self._eval_data_votes(loader, learned_indices, max_class_num, save_dir)
        steps = range(830, 940, 30)
        with torch.no_grad():
            if learned_indices is None:
                merged = {}
                for t in steps:
                    for batch_data in loader:
                        for _ in range(5):
                            for key, v in self.label_batch(batch_data, None, t=t).items():
                                merged.setdefault(key, []).extend(v)
                learned_indices = []
                for i in range(max_class_num + 1):
                    if '%d_%d' % (i - 1, i) in merged:
                        continue
                    key = '%d_%d' % (i, i + 1)
                    if key in merged:
                        num1, num2 = Counter(merged[key]).most_common()[0][0].split('_')
                        learned_indices += [int(num1), int(num2)]
                    else:
                        learned_indices.append(i)
                return learned_indices
            for batch_data in loader:
                votes = {}
                for t in steps:
                    for _ in range(41):
                        outs, file_ids = self.label_batch(batch_data, learned_indices, t=t, label_mode=True)
                        for fid, o in zip(file_ids, outs):
                            votes.setdefault(fid, []).append(o)
                for key, v in votes.items():
                    with open(os.path.join(save_dir, key + '.txt'), 'w') as f:
                        f.write(str(Counter(v).most_common()[0][0]))
