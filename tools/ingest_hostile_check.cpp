/* ingest_hostile_check.cpp -- the hostile-input cases of tests/ingest_hostile.py under the host sanitizers: a stand-alone program,
 * compiled TOGETHER with duet_ingest.cpp and run on the CPU (`make -C duet_amd/csrc ingest_check` builds both binaries):
 *     python -m tests.ingest_hostile /tmp/hostile
 *     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Iinclude \
 *         tools/ingest_hostile_check.cpp duet_amd/csrc/duet_ingest.cpp -o ingest_hostile_check_asan -lz -lpthread
 *     ./ingest_hostile_check_asan /tmp/hostile/manifest.tsv
 *     g++ -O1 -g -std=c++17 -fsanitize=thread -fno-omit-frame-pointer -Iinclude tools/ingest_hostile_check.cpp \
 *         duet_amd/csrc/duet_ingest.cpp -o ingest_hostile_check_tsan -lz -lpthread
 *     ./ingest_hostile_check_tsan /tmp/hostile/manifest.tsv 50            (the several-contig cases 50 times each)
 * It reads the manifest (name, path, mode, expected status per line; the modes are described in tests/ingest_hostile.py), calls
 * duet_ingest_add_bam / _add_bams / _parse_vcf / _get_marks on every case, with SVIM-mode extraction off and on, checks each status
 * against the manifest and walks every array the library hands out, so that a stray read or a race is the sanitizer's to report.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "duet_ingest.h"

static int fails = 0;
static const char *cur = "";
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s: %s:%d: %s\n", cur, __FILE__, __LINE__, #x); ++fails; } } while (0)

static const char *kContigs[24] = {"1", "2", "3", "4", "5", "6", "7", "8", "9", "10", "11", "12", "13", "14", "15", "16", "17", "18",
                                   "19", "20", "21", "22", "X", "Y"};

static std::vector<std::string> split(const std::string &s, char sep)
{
    std::vector<std::string> out;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, sep)) out.push_back(item);
    return out;
}

// "threads=4:contigs=0,1" -> the value of `key`, or `dflt`
static std::string option(const std::string &mode, const std::string &key, const std::string &dflt)
{
    for (const std::string &kv : split(mode, ':'))
        if (kv.compare(0, key.size() + 1, key + "=") == 0) return kv.substr(key.size() + 1);
    return dflt;
}

static uint64_t sink = 0;
template <class T> static void walk(const T *p, size_t n) { for (size_t i = 0; i < n; ++i) sink += (uint64_t)p[i]; }

static void walk_arrays(duet_ingest *g)
{
    duet_ingest_arrays a;
    CHECK(duet_ingest_get_arrays(g, &a) == DUET_INGEST_OK);
    walk(a.cand_ctg_off, a.n_contigs + 1);
    walk(a.read_off, a.n_contigs + 1);
    walk(a.read_tag, a.n_reads);
    walk(a.cand_pos, a.n_cands);
    walk(a.cand_svlen, a.n_cands);
    walk(a.cand_svread, a.n_cands);
    walk(a.cand_refread, a.n_cands);
    walk(a.cand_gt_ok, a.n_cands);
    walk(a.cand_off, a.n_cands + 1);
    walk(a.mark_read, a.n_marks);
    for (uint32_t i = 0; i < a.n_marks; ++i) CHECK(a.mark_read[i] == 0xFFFFFFFFu || a.mark_read[i] < a.n_reads);
    duet_ingest_rows r;
    CHECK(duet_ingest_get_rows(g, &r) == DUET_INGEST_OK);
    walk(r.pool, r.pool_bytes);
    walk(r.str_off, 4 * (size_t)r.n_cands + 1);
    walk(r.cand_chrom_rank, r.n_cands);
}

static void walk_marks(duet_ingest *g)
{
    duet_ingest_marks m;
    CHECK(duet_ingest_get_marks(g, &m) == DUET_INGEST_OK);
    walk(m.mark_contig, m.n_marks);
    walk(m.mark_type, m.n_marks);
    walk(m.mark_pos, m.n_marks);
    walk(m.mark_span, m.n_marks);
    walk(m.mark_read, m.n_marks);
    walk(m.read_tag, m.n_reads);
    walk(m.read_off, m.n_contigs + 1);
    walk(m.depth_off, m.n_contigs + 1);
    walk(m.depth, m.depth_off[m.n_contigs]);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s MANIFEST [repeats of the several-contig cases]\n", argv[0]); return 2; }
    const int repeats = argc > 2 ? atoi(argv[2]) : 1;
    std::ifstream man(argv[1]);
    if (!man) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    // a small caller VCF of the tool's own, joined against whatever tables a BAM case leaves behind
    char vcf[] = "/tmp/ingest_hostile_check_XXXXXX";
    {
        const int fd = mkstemp(vcf);
        if (fd < 0) return 2;
        FILE *f = fdopen(fd, "w");
        for (int k = 1; k <= 4; ++k)
            fprintf(f, "chr%d\t1000\tid\tN\t<DEL>\t.\tPASS\tPRECISE;SVTYPE=DEL;SVLEN=-80;END=1080;RE=9;RNAMES=r1,,q0,c%d_0,zz;STRAND=+-\t"
                       "GT:DR:DV:PL:GQ\t0/1:3:9:1,2,3:9\n", k, k - 1);
        fclose(f);
    }
    std::string line;
    int n_cases = 0;
    while (std::getline(man, line)) {
        const std::vector<std::string> col = split(line, '\t');
        if (col.size() != 4) { fprintf(stderr, "bad manifest line: %s\n", line.c_str()); ++fails; continue; }
        cur = col[0].c_str();
        const std::string &path = col[1], &mode = col[2];
        const int want = atoi(col[3].c_str());
        const std::string kind = mode.substr(0, mode.find(':'));
        const int threads = atoi(option(mode, "threads", "2").c_str());
        ++n_cases;
        if (kind == "bam" || kind == "extract") {
            const uint32_t bin = (uint32_t)atol(option(mode, "bin", "1000").c_str());
            for (int extract = 0; extract < 2; ++extract) {
                if (kind == "extract" && !extract) continue;
                duet_ingest *g = duet_ingest_create(24, kContigs);
                CHECK(g != nullptr);
                if (extract) CHECK(duet_ingest_set_extraction(g, 1, 40, 20, bin) == DUET_INGEST_OK);
                const int rc = duet_ingest_add_bam(g, 0, path.c_str(), threads);
                // (with extraction on, a case of the tag path may decline for the extraction's own reasons, never worse)
                if (extract && kind == "bam" && want == DUET_INGEST_OK) CHECK(rc == DUET_INGEST_OK || rc == DUET_INGEST_UNSUPPORTED);
                else CHECK(rc == want);
                if (rc != DUET_INGEST_OK) CHECK(strlen(duet_ingest_error(g)) > 0);
                if (extract) walk_marks(g);
                if (rc == DUET_INGEST_OK) {
                    CHECK(duet_ingest_parse_vcf(g, vcf, threads) == DUET_INGEST_OK);
                    walk_arrays(g);
                }
                duet_ingest_destroy(g);
            }
        } else if (kind == "bams") {
            std::vector<std::string> paths = path == "-" ? std::vector<std::string>() : split(path, ',');
            std::vector<int> contigs;
            for (const std::string &c : split(option(mode, "contigs", ""), ',')) contigs.push_back(atoi(c.c_str()));
            CHECK(paths.size() == contigs.size());
            std::vector<const char *> ptrs;
            for (const std::string &p : paths) ptrs.push_back(p.c_str());
            for (int rep = 0; rep < repeats; ++rep) {
                duet_ingest *g = duet_ingest_create(24, kContigs);
                CHECK(g != nullptr);
                const int rc = duet_ingest_add_bams(g, (int)contigs.size(), contigs.data(), ptrs.data(), threads);
                CHECK(rc == want);
                if (rc != DUET_INGEST_OK) CHECK(strlen(duet_ingest_error(g)) > 0);
                CHECK(duet_ingest_parse_vcf(g, vcf, threads) == DUET_INGEST_OK);
                walk_arrays(g);
                duet_ingest_destroy(g);
            }
        } else if (kind == "vcf") {
            duet_ingest *g = duet_ingest_create(24, kContigs);
            CHECK(g != nullptr);
            const int rc = duet_ingest_parse_vcf(g, path.c_str(), threads);
            CHECK(rc == want);
            if (rc == DUET_INGEST_OK) walk_arrays(g);
            else CHECK(strlen(duet_ingest_error(g)) > 0);
            duet_ingest_destroy(g);
        } else {
            fprintf(stderr, "%s: unknown mode %s\n", cur, mode.c_str());
            ++fails;
        }
    }
    remove(vcf);
    if (fails) printf("FAILED (%d) over %d manifest lines\n", fails, n_cases);
    else printf("ok (%d manifest lines)\n", n_cases);
    return fails ? 1 : 0;
}
