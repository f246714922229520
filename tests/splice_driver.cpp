// splice_driver.cpp - csrc/jd_splice.h and the spliced side of csrc/jd_score_plan.h under plain g++ (tests/test_splice_cpu.py): the
// argument check, the window, the gather, the spans of a batch, the push plan driven the way jd_host_stream.h drives it, the plan.
//   check IN_DIM LEFT RIGHT      prints "rc D" and, behind a newline, the message
//   gather FRAMES N D LEFT RIGHT OUT     FRAMES: N x D raw floats, one utterance; OUT: N x (LEFT + RIGHT + 1) D raw floats
//   wave FC TILE NB START0 LEN0 START1 LEN1 ...      wave_layout with JD_FC = FC, then per entry of row_src a line "src lo hi"
//   push IN META ROWS            IN: int32 records {left, right, n, push[n]} - a stream pushed in these pieces of frames whose one value is
//                                their own number, then finished.  A twin of push_spliced (jd_host_stream.h) over plain vectors, the
//                                device's gather replaced by jd_splice_frame on the staging buffer.  META: int32 records per call (the
//                                finish included) {sequence, pushed, n_front, n_buf, n_keep, held, n_rows, row_first, lowest and highest
//                                buffer frame a window read (0, -1 without rows), chunks whose piece does not hold their windows};
//                                ROWS: per sequence, per row in the order released, int32 {frame, window[C]} - frame VALUES as read.
//   plan D N_GMM N_ROWS MAX_BLOCKS TIED BF16 SPLICED     prints kernel tile_rows grid lds_bytes
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "jd_splice.h"
#include "jd_score_plan.h"

static bool slurp(const char *path, std::vector<unsigned char> &b)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    unsigned char chunk[4096];
    size_t n;
    b.clear();
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) b.insert(b.end(), chunk, chunk + n);
    fclose(f);
    return true;
}
static bool spill(const char *path, const void *p, size_t n)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// one stream, as PushStream and push_spliced keep it; a chunk of `fc` rows goes up as jd_stream_push's loop sends it
struct Stream {
    int left, right, pushed = 0, searched = 0;
    std::vector<float> held;
};
static void push(Stream &S, int seq, int n_new, bool finishing, int fc, std::vector<int32_t> &meta, std::vector<int32_t> &rows)
{
    const SplicePush plan = splice_push_plan(S.left, S.right, S.pushed, n_new, finishing);
    std::vector<float> buf((size_t)plan.n_buf);
    for (int i = 0; i < plan.n_front; ++i) buf[(size_t)i] = S.held[S.held.size() - (size_t)plan.n_front + (size_t)i];
    for (int i = 0; i < n_new; ++i) buf[(size_t)(plan.n_front + i)] = (float)(S.pushed + i);
    int lowest = 0, highest = -1, bad_chunks = 0;
    const int C = S.left + S.right + 1;
    for (int done = 0; done < plan.n_rows; done += fc) {
        const int n = std::min(fc, plan.n_rows - done);
        int b0 = 0, b1 = 0;
        splice_rows_window(S.left, S.right, plan.span, plan.row_buf + done, n, &b0, &b1);
        if (b0 < 0 || b1 > plan.n_buf || b1 - b0 > fc + S.left + S.right) ++bad_chunks;
        const JdSpan up{0, b1 - b0 - 1};                               // the rows' spans in the piece that goes up
        for (int i = 0; i < n; ++i) {
            const int centre = plan.row_buf + done + i;
            rows.push_back((int32_t)buf[(size_t)centre]);
            for (int c = 0; c < C; ++c) {
                const int whole = jd_splice_frame(centre, c, S.left, plan.span), piece = b0 + jd_splice_frame(centre - b0, c, S.left, up);
                if (whole != piece) ++bad_chunks;
                if (highest < lowest) lowest = highest = whole;
                lowest = std::min(lowest, whole); highest = std::max(highest, whole);
                rows.push_back(whole >= 0 && whole < plan.n_buf ? (int32_t)buf[(size_t)whole] : -1);
            }
        }
    }
    S.searched += plan.n_rows;
    S.pushed += n_new;
    S.held.assign(buf.end() - plan.n_keep, buf.end());
    const int32_t m[11] = {seq, S.pushed, plan.n_front, plan.n_buf, plan.n_keep, plan.held, plan.n_rows, plan.row_first, lowest, highest, bad_chunks};
    meta.insert(meta.end(), m, m + 11);
    if (plan.held != S.pushed - S.searched || plan.buf_frame0 + plan.n_buf != S.pushed || plan.keep_first + plan.n_keep != S.pushed) meta.back() += 1000;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "check" && argc == 5) {
        char msg[300] = "";
        int D = -1;
        const int rc = jd_splice_check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), &D, msg, sizeof msg);
        printf("%d %d\n%s\n", rc, D, msg);
        return 0;
    }
    if (cmd == "gather" && argc == 8) {
        const int n = atoi(argv[3]), D = atoi(argv[4]), left = atoi(argv[5]), right = atoi(argv[6]), C = left + right + 1;
        std::vector<unsigned char> b;
        if (!slurp(argv[2], b) || b.size() != (size_t)n * D * 4) return 3;
        std::vector<float> f((size_t)n * D), x((size_t)n * C * D);     // (exact sizes: the sanitizer sees a read or a write past either)
        if (!b.empty()) memcpy(f.data(), b.data(), b.size());
        for (int r = 0; r < n; ++r) jd_splice_gather(f.data(), D, left, right, r, JdSpan{0, n - 1}, x.data() + (size_t)r * C * D);
        return spill(argv[7], x.data(), x.size() * 4) ? 0 : 3;
    }
    if (cmd == "wave" && argc >= 5) {
        const int fc = atoi(argv[2]), tile = atoi(argv[3]), nb = atoi(argv[4]);
        if (argc != 5 + 2 * nb) return 2;
        std::vector<int64_t> ustart((size_t)nb), ulen((size_t)nb);
        for (int u = 0; u < nb; ++u) { ustart[(size_t)u] = atoll(argv[5 + 2 * u]); ulen[(size_t)u] = atoll(argv[6 + 2 * u]); }
        WavePlan P;
        const WaveStatus st = wave_layout(WaveIn{nb, ustart.data(), ulen.data(), (size_t)1 << 34, 0, 7, fc, tile}, &P);
        if (st.code != WAVE_OK) return 4;
        std::vector<JdSpan> span;
        splice_wave_spans(P, ustart.data(), &span);
        if (span.size() != P.row_src.size()) return 5;
        printf("%d %d\n", P.n_chunks, P.Fc);
        for (size_t r = 0; r < span.size(); ++r) printf("%d %d %d\n", P.row_src[r], span[r].lo, span[r].hi);
        return 0;
    }
    if (cmd == "push" && argc == 5) {
        std::vector<unsigned char> b;
        if (!slurp(argv[2], b) || b.size() % 4) return 3;
        std::vector<int32_t> in(b.size() / 4), meta, rows;
        if (!b.empty()) memcpy(in.data(), b.data(), b.size());
        int seq = 0;
        for (size_t at = 0; at < in.size(); ++seq) {
            if (at + 3 > in.size() || at + 3 + (size_t)in[at + 2] > in.size()) return 3;
            Stream S{in[at], in[at + 1]};
            const int n = in[at + 2];
            // (chunks of 4 rows: a push of 5 frames, or a finish that releases more, is cut as a push of more than Fc frames is)
            for (int i = 0; i < n; ++i) push(S, seq, in[at + 3 + (size_t)i], false, 4, meta, rows);
            push(S, seq, 0, true, 4, meta, rows);
            at += 3 + (size_t)n;
        }
        return spill(argv[3], meta.data(), meta.size() * 4) && spill(argv[4], rows.data(), rows.size() * 4) ? 0 : 3;
    }
    if (cmd == "plan" && argc == 9) {
        ScorePlanIn in{atoi(argv[2]), atoi(argv[3]), true, true, false, atoi(argv[4]), atoi(argv[5]), -1, false, 0, atoi(argv[6]) != 0, atoi(argv[7]) != 0,
                       atoi(argv[8]) != 0};
        const ScorePlan p = score_plan(in);
        printf("%d %d %u %zu\n", p.kernel, p.tile_rows, p.grid, p.lds_bytes);
        return 0;
    }
    return 2;
}
