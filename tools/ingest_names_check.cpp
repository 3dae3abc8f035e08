// ingest_names_check.cpp -- a stand-alone memory check of the VCF path's mark names (duet_ingest_keep_mark_names before
// duet_ingest_parse_vcf*): compiled TOGETHER with duet_ingest.cpp under -fsanitize=address,undefined and run on the CPU,
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude tools/ingest_names_check.cpp \
//         duet_amd/csrc/duet_ingest.cpp -o ingest_names_check -lz -lpthread && ./ingest_names_check
// It writes a caller VCF of its own (three contigs, one of them empty, 5000 candidates so that the join runs on several threads,
// repeated, empty and long names), parses it with and without the opt-in, in one call and in two, and walks every name.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "duet_ingest.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

int main()
{
    char path[] = "/tmp/ingest_names_check_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) return 2;
    FILE *f = fdopen(fd, "w");
    fputs("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n", f);
    std::vector<std::string> want;              // every mark's name, file order
    std::vector<int> want_contig;
    const char *contig[2] = {"1", "3"};
    for (int k = 0; k < 2; ++k)
        for (int c = 0; c < 2500; ++c) {
            std::string names;
            const int n = 1 + c % 40;               // more than one batch of 32 lookups now and then
            for (int i = 0; i < n; ++i) {
                std::string nm = (c % 7 == 0 && i == 1) ? std::string() : "read_" + std::to_string((c * 3 + i * i) % 900);
                if (c % 100 == 0 && i == 0) nm.assign(300, 'x');
                if (i) names += ',';
                names += nm;
                want.push_back(nm);
                want_contig.push_back(k);
            }
            fprintf(f, "%s\t%d\tid\tN\t<DEL>\t.\tPASS\tPRECISE;SVTYPE=DEL;SVLEN=-80;END=180;RE=5;RNAMES=%s;STRAND=+-\tGT:DR:DV:PL:GQ\t0/1:3:5:1,2,3:9\n",
                    contig[k], 100 + c, names.c_str());
        }
    fclose(f);

    const char *labels[3] = {"1", "2", "3"};
    for (int two_calls = 0; two_calls < 2; ++two_calls) {
        duet_ingest *g = duet_ingest_create(3, labels);
        CHECK(g != nullptr);
        duet_ingest_mark_names nm;
        CHECK(duet_ingest_get_mark_names(g, &nm) != DUET_INGEST_OK);
        CHECK(duet_ingest_keep_mark_names(g, 1) == DUET_INGEST_OK);
        for (int round = 0; round < 2; ++round) {               // the second parse starts the names afresh
            if (two_calls) {
                CHECK(duet_ingest_parse_vcf_begin(g, path, 4) == DUET_INGEST_OK);
                CHECK(duet_ingest_parse_vcf_finish(g) == DUET_INGEST_OK);
            } else {
                CHECK(duet_ingest_parse_vcf(g, path, 4) == DUET_INGEST_OK);
            }
            duet_ingest_arrays a;
            CHECK(duet_ingest_get_arrays(g, &a) == DUET_INGEST_OK);
            CHECK(duet_ingest_get_mark_names(g, &nm) == DUET_INGEST_OK);
            CHECK(nm.n_marks == a.n_marks && nm.n_marks == want.size());
            CHECK(nm.name_off[0] == 0 && nm.name_off[nm.n_names] == nm.pool_bytes);
            size_t same = 0;
            for (uint32_t i = 0; i < nm.n_marks && i < want.size(); ++i) {
                const uint32_t j = nm.mark_name[i];
                if (j >= nm.n_names) { CHECK(j < nm.n_names); break; }
                const std::string got(nm.name_pool + nm.name_off[j], nm.name_pool + nm.name_off[j + 1]);
                same += got == want[i];
                CHECK(a.mark_read[i] == 0xFFFFFFFFu);           // (no BAM was added: nobody is tagged, everybody has a name)
            }
            CHECK(same == want.size());
            // interned per contig: the entries of contig 1 come before those of contig 3, none is shared
            uint32_t top0 = 0, low1 = 0xFFFFFFFFu;
            for (uint32_t i = 0; i < nm.n_marks; ++i) {
                if (want_contig[i] == 0) top0 = nm.mark_name[i] > top0 ? nm.mark_name[i] : top0;
                else low1 = nm.mark_name[i] < low1 ? nm.mark_name[i] : low1;
            }
            CHECK(top0 < low1);
        }
        CHECK(duet_ingest_keep_mark_names(g, 0) != DUET_INGEST_OK);       // too late
        duet_ingest_destroy(g);
    }
    {   // without the opt-in nothing is kept
        duet_ingest *g = duet_ingest_create(3, labels);
        CHECK(duet_ingest_parse_vcf(g, path, 4) == DUET_INGEST_OK);
        duet_ingest_mark_names nm;
        CHECK(duet_ingest_get_mark_names(g, &nm) != DUET_INGEST_OK);
        duet_ingest_destroy(g);
    }
    remove(path);
    printf(fails ? "FAILED (%d)\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
