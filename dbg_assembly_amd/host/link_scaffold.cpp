// link_scaffold -- the link_scaffold module's scaffolder (link_scaffold/link_scaffold.cpp + link_func.cpp) with the link table built
// and the scaffold sequences written on the GPU (LINK section of include/dbgk.h).  Same command line, same six output files
// <prefix>.insert<I>.scaffold.{links.all,links.uniq,pos.tab,seq.fa} and .scaffold_repeat.{seq.fa,pos.tab}, same protocol on stderr.
#include <unistd.h>
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "dbgk.h"

using namespace std;

static string Output_prefix = "Output";
static int InsertSize = 400;
static int PairNumCut = 3;
static int IsMatePair = 0;

static const size_t BatchRecords = 1 << 22; // records per device batch

static void die(const char *what, int rc)
{
	cerr << what << " failed: " << dbgk_strerror(rc);
	if (rc == DBGK_ERR_HIP) cerr << " [" << dbgk_last_error() << "]";
	cerr << endl;
	exit(1);
}

static void usage()
{
	cout << "\nFunction instruction:\nlink_scaffold, converts read PEs into contig relations, links the contigs into scaffolds.\
\n(1) If two contigs are neighbor, and they are in the same DNA strand, a pair of PE read will mapped in\
   the F and R way, that is, one read mapped forwardly on one contig, and the other read mapped reversely\
   on the other contig. We use this character to decide the strand relations between two neighbor contigs.\
\n(2) Each contig has two strand forms, we stored both of them in the memory, and each contig node only\
   has one link, the 3'-direction. This can make the strand problem quite easy, and do not increase the\
   memory usage too much.\
\n(3) This program require more than a specified number of read pairs to support two neighbor contigs,\
   and build a graph using neighboring-link-technology, take contig as nodes, and the 3'-link as arcs.\
\n(4) The scaffold sequences were read out from a linear contig, that is, with only one ingoing arc and one\
   outgoing arc, and scaffolding stops at breaking or branching nodes.\n";
	cout << "\nlink_scaffold  <contig_file.fa>  <mapping_twoctg_files.lib>\n"
	     << "   Function: link contigs into scaffolds by pair-end or mate-pair reads, inside gap are not filled" << endl
	     << "   Version: 1.0" << endl
	     << "   -m <int>   input mapping data type: 0, pair-ends; 1. mated-pair,  default=" << IsMatePair << endl
	     << "   -n <int>   the minimum number of read-pairs required to support a link between two contigs, default=" << PairNumCut << endl
	     << "   -i <int>   mean insert size for pair-ends or mated-pair reads, default=" << InsertSize << endl
	     << "   -o <str>   the output file prefix, set in commond-line, default = " << Output_prefix << endl
	     << "   -h         get the help information\n" << endl;
	exit(0);
}

static void output_parameters()
{
	cerr << "link_scaffold  [version 1.0]" << endl
	     << "   -m <int>   input mapping data type: 0, pair-ends; 1. mated-pair,  default=" << IsMatePair << endl
	     << "   -n <int>   the minimum number of read pairs required to support a link between two contigs, default=" << PairNumCut << endl
	     << "   -i <int>   mean insert size for pair-ends or mated-pair reads, default=" << InsertSize << endl
	     << "   -o <str>   the output prefix, set in commond-line, default = " << Output_prefix << endl
	     << "   -h         get the help information\n" << endl;
}

// split (link_func.cpp)
static void split(const string &line, vector<string> &tokens, const char *delim)
{
	size_t i = 0;
	for (;;) {
		i = line.find_first_not_of(delim, i);
		if (i == string::npos) break;
		const size_t j = line.find_first_of(delim, i);
		tokens.push_back(line.substr(i, j == string::npos ? string::npos : j - i));
		if (j == string::npos) break;
		i = j;
	}
}

// reading_para_file (link_func.cpp:75-95)
static void reading_para_file(const string &para_file, vector<string> &files)
{
	ifstream infile(para_file.c_str());
	if (!infile) cerr << "fail to open input file" << para_file << endl;
	string line;
	while (getline(infile, line, '\n')) {
		if (!line.empty() && line[0] == '#') continue;
		vector<string> vec_line;
		split(line, vec_line, " \t\n");
		if (vec_line.empty()) continue;
		files.push_back(vec_line[0]);
	}
}

// read_contig_file (link_func.cpp:99-136) without the empty strings of the even nodes: contig c is node 2c + 1
static void read_contig_file(const string &file, vector<string> &seqs, vector<string> &ids)
{
	ifstream infile(file.c_str());
	if (!infile) cerr << "fail to open input file " << file << endl;
	string contig_str, line;
	while (getline(infile, line, '\n')) {
		if (!line.empty() && line[0] == '>') {
			vector<string> vec_head;
			split(line, vec_head, "> \t");
			ids.push_back(vec_head.empty() ? string() : vec_head[0]);
			if (contig_str.size() > 0) seqs.push_back(contig_str);
			contig_str.clear();
		} else {
			contig_str += line;
		}
	}
	if (contig_str.size() > 0) seqs.push_back(contig_str);
}

// ctgStr2Id (link_func.h:130)
static int ctgStr2Id(const string &s) { return s.size() > 4 ? atoi(s.c_str() + 4) : 0; }

// getline over a plain or gzip file (what igzstream + getline read)
struct LineReader {
	gzFile f = nullptr;
	vector<char> buf = vector<char>(1 << 20);
	size_t pos = 0, len = 0;
	bool eof = false;
	explicit LineReader(const string &path)
	{
		f = gzopen(path.c_str(), "rb");
		if (!f) cerr << "fail to open input file " << path << endl;
		else gzbuffer(f, 1 << 20);
	}
	~LineReader() { if (f) gzclose(f); }
	bool getline(string &s)
	{
		s.clear();
		bool any = false;
		for (;;) {
			if (pos == len) {
				if (eof || !f) return any;
				const int n = gzread(f, buf.data(), (unsigned)buf.size());
				if (n <= 0) { eof = true; return any; }
				pos = 0;
				len = (size_t)n;
			}
			any = true;
			const char *b = buf.data() + pos;
			const char *nl = (const char *)memchr(b, '\n', len - pos);
			if (nl) {
				s.append(b, nl - b);
				pos += (nl - b) + 1;
				return true;
			}
			s.append(b, len - pos);
			pos = len;
		}
	}
};

// the fields parse_pair_ends_map_file / parse_mate_pairs_map_file take from one line (link_func.cpp:253-260)
static void parse_map_file(const string &file, dbgk_link *L, size_t n_contigs)
{
	LineReader in(file);
	vector<dbgk_link_pair> batch;
	batch.reserve(BatchRecords);
	auto flush = [&]() {
		const int rc = dbgk_link_add_pairs(L, batch.data(), batch.size());
		if (rc) die("dbgk_link_add_pairs", rc);
		batch.clear();
	};
	string line;
	vector<string> v;
	while (in.getline(line)) {
		if (!line.empty() && line[0] == '#') continue;
		v.clear();
		split(line, v, " \t\n");
		if (v.size() < 19) { // the reference reads vec_line[18] whatever the line holds
			if (v.empty()) continue;
			cerr << "link_scaffold: a line of " << file << " has " << v.size() << " fields, 19 are needed" << endl;
			exit(1);
		}
		const int id1 = ctgStr2Id(v[4]), id2 = ctgStr2Id(v[14]);
		if (id1 % 2 != 1 || id2 % 2 != 1 || id1 < 1 || id2 < 1 || (size_t)(id1 / 2) >= n_contigs || (size_t)(id2 / 2) >= n_contigs) {
			cerr << "link_scaffold: " << v[4] << " / " << v[14] << " in " << file << " is no contig of the contig file" << endl;
			exit(1);
		}
		dbgk_link_pair r{};
		r.contig1 = id1 / 2; r.start1 = atoi(v[6].c_str()); r.end1 = atoi(v[7].c_str());
		r.contig2 = id2 / 2; r.start2 = atoi(v[16].c_str()); r.end2 = atoi(v[17].c_str());
		r.direct1 = v[8].size() == 1 ? (uint8_t)v[8][0] : (uint8_t)'?';
		r.direct2 = v[18].size() == 1 ? (uint8_t)v[18][0] : (uint8_t)'?';
		batch.push_back(r);
		if (batch.size() >= BatchRecords) flush();
	}
	flush();
}

// display_data_in_link (link_func.cpp:515-537)
static void display_data_in_link(dbgk_link *L, int stage, const vector<uint64_t> &first, const string &file)
{
	const size_t n_nodes = first.size() - 1;
	vector<uint8_t> inlink(n_nodes), link(n_nodes);
	vector<dbgk_link_entry> e(first[n_nodes] + 1);
	const int rc = dbgk_link_snapshot(L, stage, inlink.data(), link.data(), e.data());
	if (rc) die("dbgk_link_snapshot", rc);
	FILE *out = fopen(file.c_str(), "w");
	if (!out) {
		cerr << "fail to open file" << file << endl;
		return;
	}
	fputs("ctg_id\tincoming_link_num\toutgoing_link_num\tlinked_id,pair_num,sum_size,avg_size;\n", out);
	for (size_t i = 1; i < n_nodes; i++) {
		fprintf(out, "%zu\t%d\t%d", i, (int)inlink[i], (int)link[i]);
		for (uint64_t j = first[i]; j < first[i + 1]; j++)
			if (e[j].freq > 0)
				fprintf(out, "\t%u,%u,%lld,%lld", e[j].target, e[j].freq, (long long)e[j].size, (long long)(e[j].size / (int64_t)e[j].freq));
		fputc('\n', out);
	}
	fclose(out);
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "m:n:i:o:h")) != -1) {
		switch (c) {
			case 'm': IsMatePair = atoi(optarg); break;
			case 'n': PairNumCut = atoi(optarg); break;
			case 'i': InsertSize = atoi(optarg); break;
			case 'o': Output_prefix = optarg; break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 3 || argc - optind < 2) usage();
	output_parameters();
	const string contig_seq_file = argv[optind++];
	const string para_map_file = argv[optind++];

	const clock_t time_start = clock();
	auto run_time = [&]() { cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl; };
	cerr << "\nProgram start ............" << endl;
	run_time();

	vector<string> contig_ids, contig_seqs;
	read_contig_file(contig_seq_file, contig_seqs, contig_ids);
	const size_t n_contigs = contig_seqs.size();
	uint64_t contig_total_num = n_contigs, contig_total_len = 0;
	vector<uint32_t> lens(n_contigs);
	for (size_t i = 0; i < n_contigs; i++) {
		if (contig_seqs[i].size() >= (1ull << 31)) {
			cerr << "link_scaffold: contig " << contig_ids[i] << " is longer than 2^31 - 1 bases" << endl;
			return 1;
		}
		lens[i] = (uint32_t)contig_seqs[i].size();
		contig_total_len += contig_seqs[i].size();
	}
	// the reference finds a contig's node through the number in its name: anything but 2c + 1 for contig c is undefined there
	if (contig_ids.size() != n_contigs) {
		cerr << "link_scaffold: " << contig_seq_file << " has a record without sequence" << endl;
		return 1;
	}
	for (size_t i = 0; i < n_contigs; i++)
		if (ctgStr2Id(contig_ids[i]) < 0 || (size_t)ctgStr2Id(contig_ids[i]) != 2 * i + 1) {
			cerr << "link_scaffold: contig " << i + 1 << " of " << contig_seq_file << " is named " << contig_ids[i] << ", its number must be "
			     << 2 * i + 1 << " (the contig stage and link_scaffold number contigs 1, 3, 5, ...)" << endl;
			return 1;
		}
	cerr << "\nInput contig number: " << contig_total_num << endl;
	cerr << "Input contig length: " << contig_total_len << endl;
	cerr << "Read contigs into memory finished !" << endl;

	vector<string> Paired_map_files;
	reading_para_file(para_map_file, Paired_map_files);
	cerr << "\nInput reads mapping files number: " << Paired_map_files.size() << endl;
	run_time();

	if (IsMatePair != 0 && IsMatePair != 1) { // the reference parses nothing then
		cerr << "link_scaffold: -m must be 0 or 1" << endl;
		return 1;
	}
	dbgk_link *L = nullptr;
	dbgk_link_params P{IsMatePair, PairNumCut, InsertSize};
	int rc = dbgk_link_create(&P, 0, &L);
	if (rc) die("dbgk_link_create", rc);
	if ((rc = dbgk_link_set_contigs(L, lens.data(), n_contigs))) die("dbgk_link_set_contigs", rc);
	for (size_t i = 0; i < Paired_map_files.size(); i++) {
		cerr << "\nparse map file: " << Paired_map_files[i] << endl;
		parse_map_file(Paired_map_files[i], L, n_contigs);
	}
	if ((rc = dbgk_link_build(L))) die("dbgk_link_build", rc);
	cerr << "\nParsed the map files done !" << endl;
	run_time();

	const size_t n_nodes = 2 * n_contigs + 1;
	vector<uint64_t> first(n_nodes + 1);
	uint64_t n_links = 0;
	dbgk_link_counters ctr{};
	if ((rc = dbgk_link_export(L, first.data(), nullptr, 0, &n_links, &ctr))) die("dbgk_link_export", rc);
	cerr << "\nFR_link_num: " << ctr.fr << endl;
	cerr << "RF_link_num: " << ctr.rf << endl;
	cerr << "FF_link_num: " << ctr.ff << endl;
	cerr << "RR_link_num: " << ctr.rr << endl;
	cerr << "Effect_link_num: " << ctr.fr + ctr.rf + ctr.ff + ctr.rr << endl;
	cerr << "Wrong_link_num: " << ctr.wrong << endl;

	dbgk_link_summary S{};
	if ((rc = dbgk_link_resolve(L, &S))) die("dbgk_link_resolve", rc);
	cerr << "\nRemoved LowFreq link num: " << S.lowfreq << endl;
	{
		vector<uint8_t> link(n_nodes);
		if ((rc = dbgk_link_snapshot(L, 0, nullptr, link.data(), nullptr))) die("dbgk_link_snapshot", rc);
		uint64_t total_link_num = 0, uniq_link_num = 0, multiple_link_num = 0, empty_link_num = 0;
		for (size_t i = 1; i < n_nodes; i += 2) {
			if (link[i] == 0) empty_link_num++;
			else if (link[i] == 1) uniq_link_num++;
			else multiple_link_num++;
			total_link_num++;
		}
		cerr << "Number and ratio of contigs having a unique 3'-link: " << uniq_link_num << "  " << (float)uniq_link_num / total_link_num << endl;
		cerr << "Number and ratio of contigs having multiple 3'-link: " << multiple_link_num << "  " << (float)multiple_link_num / total_link_num << endl;
		cerr << "Number and ratio of contigs having zero 3'-link:     " << empty_link_num << "  " << (float)empty_link_num / total_link_num << endl;
	}
	const string stem = Output_prefix + ".insert" + to_string(InsertSize);
	display_data_in_link(L, 0, first, stem + ".scaffold.links.all");
	cerr << "\nRemoved interleave links num: " << S.interleave << endl;
	cerr << "\nRemoved repeat nodes num: " << S.repeat_nodes << endl;
	cerr << "\nRemoved links [related with repeat or small nodes] num: " << S.deleted << endl;
	display_data_in_link(L, 1, first, stem + ".scaffold.links.uniq");

	// read_out_scaffold (link_scaffold.cpp:300-423): the layout comes sorted, the sequences of all scaffolds from one device call
	vector<uint64_t> scaf_first(S.scaffolds + 1);
	vector<dbgk_link_item> items(S.items + 1);
	vector<int32_t> repeats(S.repeat_nodes + 1);
	if ((rc = dbgk_link_layout(L, scaf_first.data(), items.data(), repeats.data()))) die("dbgk_link_layout", rc);
	string bases;
	vector<uint64_t> offsets(1, 0);
	bases.reserve(contig_total_len);
	for (const string &s : contig_seqs) {
		bases += s;
		offsets.push_back(bases.size());
	}
	uint64_t seq_len = 0;
	if ((rc = dbgk_link_emit(L, bases.data(), offsets.data(), n_contigs, items.data(), S.items, nullptr, 0, &seq_len)) && rc != DBGK_ERR_CAPACITY)
		die("dbgk_link_emit", rc);
	string seq(seq_len, '\0');
	if (seq_len && (rc = dbgk_link_emit(L, bases.data(), offsets.data(), n_contigs, items.data(), S.items, &seq[0], seq_len, &seq_len)))
		die("dbgk_link_emit", rc);

	ofstream ScafPosFile((stem + ".scaffold.pos.tab").c_str());
	if (!ScafPosFile) cerr << "fail to open file" << stem + ".scaffold.pos.tab" << endl;
	ofstream ScafSeqFile((stem + ".scaffold.seq.fa").c_str());
	if (!ScafSeqFile) cerr << "fail to open file" << stem + ".scaffold.seq.fa" << endl;
	uint64_t total_scaffold_len = 0, total_scaffold_lenwogap = 0, contig_included_num = 0, contig_included_len = 0;
	int scaffold_id = -1;
	uint64_t seq_pos = 0;
	for (uint64_t s = 0; s < S.scaffolds; s++) {
		scaffold_id += 2;
		int scaf_ctg_num = 0, scaf_len = 0, scaf_lenwogap = 0;
		string pos;
		for (uint64_t t = scaf_first[s]; t < scaf_first[s + 1]; t++) {
			const dbgk_link_item &it = items[t];
			const int block_start = scaf_len + 1;
			if (it.contig >= 0) {
				const int block_size = (int)lens[it.contig];
				scaf_ctg_num++;
				scaf_len += block_size;
				scaf_lenwogap += block_size;
				pos += "\t" + contig_ids[it.contig] + "\t" + to_string(block_start) + "\t" + to_string(scaf_len) + "\t" + to_string(block_size) + "\t" +
				       (it.value ? "R" : "F") + "\n";
				contig_included_num++;
				contig_included_len += block_size;
			} else {
				scaf_len += it.value;
				pos += "\tgap\t" + to_string(block_start) + "\t" + to_string(scaf_len) + "\t" + to_string(it.value) + "\tN\n";
			}
		}
		ScafSeqFile << ">scf_" << scaffold_id << "   fragment_num:" << scaf_ctg_num << "   length:" << scaf_len << "   lenwogap:" << scaf_lenwogap << "\n";
		ScafSeqFile.write(seq.data() + seq_pos, scaf_len);
		ScafSeqFile << "\n";
		seq_pos += (uint64_t)scaf_len;
		ScafPosFile << ">scf_" << scaffold_id << "\n" << pos;
		total_scaffold_len += scaf_len;
		total_scaffold_lenwogap += scaf_lenwogap;
	}
	ScafPosFile.close();
	ScafSeqFile.close();

	ofstream SingletFile((stem + ".scaffold_repeat.seq.fa").c_str());
	if (!SingletFile) cerr << "fail to open file" << stem + ".scaffold_repeat.seq.fa" << endl;
	ofstream SingletPosFile((stem + ".scaffold_repeat.pos.tab").c_str());
	if (!SingletPosFile) cerr << "fail to open file" << stem + ".scaffold_repeat.pos.tab" << endl;
	uint64_t contig_excluded_num = 0, contig_excluded_len = 0;
	for (uint64_t r = 0; r < S.repeat_nodes; r++) {
		const int32_t ctg = repeats[r];
		const uint64_t len = lens[ctg];
		scaffold_id += 2;
		SingletFile << ">scf_" << scaffold_id << "   fragment_num:1   length:" << len << "   lenwogap:" << len << "   RepeatNode\n" << contig_seqs[ctg] << "\n";
		SingletPosFile << ">scf_" << scaffold_id << "\n\t" << contig_ids[ctg] << "\t1\t" << len << "\t" << len << "\tF\n";
		contig_excluded_num++;
		contig_excluded_len += len;
	}

	cerr << "\nRead out scaffold sequence done" << endl;
	cerr << "\nTotal scaffold number:          " << S.scaffolds << endl;
	cerr << "Total scaffold length[WithGap]: " << total_scaffold_len << endl;
	cerr << "Total scaffold length[NoGap]:   " << total_scaffold_lenwogap << endl;
	cerr << "\nIncluded contig number: " << contig_included_num << "  " << (float)contig_included_num / contig_total_num << endl;
	cerr << "Included contig length: " << contig_included_len << "  " << (float)contig_included_len / contig_total_len << endl;
	cerr << "Excluded repeat contig number: " << contig_excluded_num << "  " << (float)contig_excluded_num / contig_total_num << endl;
	cerr << "Excluded repeat contig length: " << contig_excluded_len << "  " << (float)contig_excluded_len / contig_total_len << endl;
	cerr << "\nProgram finished !" << endl;
	run_time();
	dbgk_link_destroy(L);
	return 0;
}
